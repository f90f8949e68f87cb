// poison_env.h -- the switch of the workspace poison: SPERR_HIP_POISON=<byte>, decimal or 0x..,
// 0 to 255.  With it set every device buffer an engine holds is filled with that byte before a call carves it, so that
// a kernel that reads a workspace word this call did not write, and no clear covers, reads the poison and not what an
// earlier call happened to leave there.  Host only, no HIP: tests/cpp/poison_env_check.cpp runs the parser alone.
#ifndef SPERR_AMD_POISON_ENV_H
#define SPERR_AMD_POISON_ENV_H

#include <cstdlib>

namespace sperrhip {

// the byte `v` names, or -1 (off): null, empty, not a number all through, a sign, or a value past 255
inline int poison_parse(const char* v)
{
  if (!v || !*v)
    return -1;
  int base = 10;
  if (v[0] == '0' && (v[1] == 'x' || v[1] == 'X')) {
    base = 16;
    v += 2;
    if (!*v)
      return -1;
  }
  int val = 0;
  for (; *v; v++) {
    int d = -1;
    if (*v >= '0' && *v <= '9')
      d = *v - '0';
    else if (base == 16 && *v >= 'a' && *v <= 'f')
      d = *v - 'a' + 10;
    else if (base == 16 && *v >= 'A' && *v <= 'F')
      d = *v - 'A' + 10;
    if (d < 0)
      return -1;
    val = val * base + d;
    if (val > 255)
      return -1;
  }
  return val;
}

// read on every call, as SPERR_HIP_ARENA_MAX_MB is: a test changes it between calls
inline int poison_env()
{
  return poison_parse(getenv("SPERR_HIP_POISON"));
}

}  // namespace sperrhip

#endif
