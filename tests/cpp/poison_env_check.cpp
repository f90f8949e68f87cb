// poison_env_check.cpp -- the parser of the workspace poison switch (sperr_amd/csrc/poison_env.h), a program of its own:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I sperr_amd/csrc tests/cpp/poison_env_check.cpp
// The switch is a byte, decimal or 0x.., 0 to 255; anything else -- unset, empty, out of range, not a number all
// through -- is "off" (-1).  poison_env() reads the environment on every call.
#include <cstdio>
#include <cstdlib>

#include "poison_env.h"

using sperrhip::poison_env;
using sperrhip::poison_parse;

static int fails = 0;

static void expect(const char* text, int want)
{
  const int got = poison_parse(text);
  if (got != want) {
    printf("poison_parse(%s%s%s) = %d, expected %d\n", text ? "\"" : "", text ? text : "null", text ? "\"" : "", got, want);
    fails++;
  }
}

static void expect_env(const char* text, int want)
{
  if (text)
    setenv("SPERR_HIP_POISON", text, 1);
  else
    unsetenv("SPERR_HIP_POISON");
  const int got = poison_env();
  if (got != want) {
    printf("SPERR_HIP_POISON=%s: poison_env() = %d, expected %d\n", text ? text : "(unset)", got, want);
    fails++;
  }
}

int main()
{
  // accepted
  expect("0", 0);
  expect("90", 90);
  expect("255", 255);
  expect("0x5a", 0x5a);
  expect("0XFF", 0xff);
  expect("0x0", 0);
  expect("007", 7);
  expect("0x00ff", 0xff);
  // off
  expect(nullptr, -1);
  expect("", -1);
  expect("256", -1);
  expect("-1", -1);
  expect("0x100", -1);
  expect("zz", -1);
  expect("5a", -1);
  expect("0x", -1);
  expect("+5", -1);
  expect(" 5", -1);
  expect("5 ", -1);
  expect("0x5g", -1);
  expect("99999999999999999999999999", -1);   // (nothing wraps on the way to "too large")
  expect("0xffffffffffffffffffffff", -1);
  // every byte, both ways of writing it
  for (int v = 0; v < 256; v++) {
    char dec[16], hex[16];
    snprintf(dec, sizeof dec, "%d", v);
    snprintf(hex, sizeof hex, "0x%x", v);
    expect(dec, v);
    expect(hex, v);
  }
  // the environment is read on every call: a test changes it between calls
  expect_env(nullptr, -1);
  expect_env("0x5a", 0x5a);
  expect_env("255", 255);
  expect_env("", -1);
  expect_env("256", -1);
  expect_env(nullptr, -1);
  if (fails) {
    printf("poison_env_check: %d failures\n", fails);
    return 1;
  }
  printf("poison_env_check ok\n");
  return 0;
}
