// pix_planes_check -- the per-thread arithmetic of k_emit_pixels (sperr_amd/csrc/pix_planes.h) on the host, against the
// per-sample definitions the kernel used before it held plane masks: the bit-sliced msb + 1 with its seven-mask
// comparison, bit pl of a magnitude by a shift, and the loop that put one sign behind one token per turn.
//
//   pix_planes_check transpose | recurrence | signs
//
// Exit code 0 and "ok": everything agreed bit for bit.  Built with the address / undefined sanitizers.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "pix_planes.h"

using namespace sperrhip;

static int fails = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      if (fails < 20)                                                  \
        std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      fails++;                                                         \
    }                                                                  \
  } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// ---- the definitions the kernel had ---------------------------------------------------------------------------
static int msb_of(uint32_t mag) { return mag ? 31 - __builtin_clz(mag) : -1; }   // (k_quantize: 63 - clzll, -1 of zero)

static void old_above_equal(const uint32_t (&X)[7], uint32_t t, uint32_t& gt, uint32_t& eq)
{
  gt = 0;
  eq = 0xffffu;
  for (int j = 6; j >= 0; j--) {
    if ((t >> j) & 1u)
      eq &= X[j];
    else {
      gt |= eq & X[j];
      eq &= ~X[j];
    }
  }
}

static void old_masks(const uint32_t (&mag)[16], int pl, uint32_t& gtM, uint32_t& eqM, uint32_t& cbit)
{
  uint32_t M[7];
  for (int j = 0; j < 7; j++) {
    M[j] = 0;
    for (int k = 0; k < 16; k++)
      M[j] |= (((uint32_t)(msb_of(mag[k]) + 1) >> j) & 1u) << k;
  }
  old_above_equal(M, (uint32_t)pl + 1u, gtM, eqM);
  cbit = 0;
  for (int k = 0; k < 16; k++)
    cbit |= (uint32_t)((mag[k] >> pl) & 1) << k;
}

static void old_signs(uint32_t tok, uint32_t sgn, uint32_t nl, uint32_t& lval, uint32_t& lbits)
{
  lbits = nl;
  lval = tok;
  for (uint32_t rest = tok; rest;) {
    const uint32_t i = 31u - (uint32_t)__builtin_clz(rest);
    rest &= ~(1u << i);
    const uint32_t low = lval & ((2u << i) - 1u);
    lval = low | (((sgn >> i) & 1u) << (i + 1)) | ((i + 1 < 32 ? lval >> (i + 1) : 0u) << (i + 2));
    lbits++;
  }
}

// ---- transpose ------------------------------------------------------------------------------------------------
static void check_transpose_of(const uint32_t (&mag)[16])
{
  uint32_t P[16];
  std::memcpy(P, mag, sizeof(P));
  pix_transpose16(P);
  for (int pl = 0; pl < 32; pl++) {
    const uint32_t c = pix_plane(P, pl);
    CHECK(c <= 0xffffu);
    for (int k = 0; k < 16; k++)
      CHECK(((c >> k) & 1u) == ((mag[k] >> pl) & 1u));
  }
}

static void check_transpose()
{
  uint32_t mag[16];
  for (int rep = 0; rep < 20000; rep++) {
    for (int k = 0; k < 16; k++)
      mag[k] = (uint32_t)rnd() >> (rnd() % 33 == 32 ? 31 : rnd() % 32);   // every width, not only full ones
    check_transpose_of(mag);
  }
  std::memset(mag, 0, sizeof(mag));
  check_transpose_of(mag);
  std::memset(mag, 0xff, sizeof(mag));
  check_transpose_of(mag);
  const int planes[4] = {0, 15, 16, 31};
  for (int pl : planes)
    for (int k = 0; k < 16; k++) {   // a single bit in the whole matrix
      std::memset(mag, 0, sizeof(mag));
      mag[k] = 1u << pl;
      check_transpose_of(mag);
    }
  for (int pl : planes) {            // the plane set in every sample and nothing else
    for (int k = 0; k < 16; k++)
      mag[k] = 1u << pl;
    check_transpose_of(mag);
  }
  for (int k = 0; k < 16; k++) {     // one sample with bit 31 among zeros, with and without bits below it
    std::memset(mag, 0, sizeof(mag));
    mag[k] = 0x80000000u;
    check_transpose_of(mag);
    mag[k] = 0x80000000u | (uint32_t)rnd();
    check_transpose_of(mag);
  }
}

// ---- recurrence -----------------------------------------------------------------------------------------------
static void check_recurrence_of(const uint32_t (&mag)[16])
{
  uint32_t P[16];
  std::memcpy(P, mag, sizeof(P));
  pix_transpose16(P);
  uint32_t gt = 0;   // nothing has its msb above plane 31
  for (int p = 31; p >= 0; p--) {
    uint32_t gtOld, eqOld, cbitOld, eq;
    old_masks(mag, p, gtOld, eqOld, cbitOld);
    const uint32_t c = pix_plane(P, p);
    CHECK(gt == gtOld);
    pix_msb_step(c, gt, eq);
    CHECK(eq == eqOld);
    CHECK(c == cbitOld);
  }
  uint32_t nz = 0;
  for (int k = 0; k < 16; k++)
    nz |= (uint32_t)(mag[k] != 0) << k;
  CHECK(gt == nz);   // below plane 0: every sample that is not zero
}

static void check_recurrence()
{
  uint32_t mag[16];
  for (int rep = 0; rep < 20000; rep++) {
    for (int k = 0; k < 16; k++) {
      const uint32_t r = (uint32_t)rnd();
      const uint32_t w = (uint32_t)(rnd() % 34);   // msb -1 (zero) .. 31, zeros more often than chance would have them
      mag[k] = w >= 32 ? 0u : (r | 0x80000000u) >> (31 - w);
    }
    if (rep % 7 == 0)
      mag[rnd() % 16] = 0;
    check_recurrence_of(mag);
  }
  std::memset(mag, 0, sizeof(mag));
  check_recurrence_of(mag);
  std::memset(mag, 0xff, sizeof(mag));
  check_recurrence_of(mag);
  for (int k = 0; k < 16; k++)
    mag[k] = 1u << (2 * k + (k & 1));
  check_recurrence_of(mag);
}

// ---- tables, pext, sign expansion --------------------------------------------------------------------------------
static uint8_t pextLut[256], signLut[256];

static void check_signs_of(uint32_t tok, uint32_t sgn, uint32_t nl)
{
  uint32_t want, wantBits;
  old_signs(tok, sgn, nl, want, wantBits);
  const uint32_t got = pix_sign_expand(signLut, tok, sgn);
  const uint32_t gotBits = nl + (uint32_t)__builtin_popcount(tok);
  CHECK(got == want);
  CHECK(gotBits == wantBits);
  CHECK(gotBits == 32 || (got >> gotBits) == 0);
}

static void check_signs()
{
  for (uint32_t i = 0; i < 256; i++) {
    pextLut[i] = pix_pext_entry(i >> 4, i & 15u);
    signLut[i] = pix_sign_entry(i >> 4, i & 15u);
  }
  // every (token nibble, sign nibble) pair: value and length of the entry, and the expansion of four tokens
  for (uint32_t tn = 0; tn < 16; tn++)
    for (uint32_t sn = 0; sn < 16; sn++) {
      uint32_t want, wantBits;
      old_signs(tn, sn, 4, want, wantBits);
      CHECK(signLut[tn * 16 + sn] == want);
      CHECK(4u + (uint32_t)__builtin_popcount(tn) == wantBits);
      check_signs_of(tn, sn, 4);
    }
  // every 16-bit token word against 64 random sign words (the signs of tokens that are '0' must not matter)
  for (uint32_t tok = 0; tok < 65536; tok++)
    for (int r = 0; r < 64; r++)
      check_signs_of(tok, (uint32_t)rnd() & 0xffffu, 16);
  for (int r = 0; r < 1000000; r++) {
    const uint32_t nl = (uint32_t)(rnd() % 17);
    const uint32_t mask = nl == 16 ? 0xffffu : (1u << nl) - 1u;
    check_signs_of((uint32_t)rnd() & mask, (uint32_t)rnd() & mask, nl);
  }
  // the pext in front of it: packed bits against a loop over the mask
  for (int r = 0; r < 1000000; r++) {
    const uint32_t val = (uint32_t)rnd() & 0xffffu, mask = (uint32_t)rnd() & 0xffffu;
    uint32_t want = 0, o = 0;
    for (int i = 0; i < 16; i++)
      if ((mask >> i) & 1u)
        want |= ((val >> i) & 1u) << o++;
    CHECK(pix_pext16(pextLut, val, mask) == want);
  }
}

int main(int argc, char** argv)
{
  const char* what = argc > 1 ? argv[1] : "";
  if (!std::strcmp(what, "transpose"))
    check_transpose();
  else if (!std::strcmp(what, "recurrence"))
    check_recurrence();
  else if (!std::strcmp(what, "signs"))
    check_signs();
  else {
    std::printf("usage: pix_planes_check transpose|recurrence|signs\n");
    return 2;
  }
  if (fails) {
    std::printf("%d checks failed\n", fails);
    return 1;
  }
  std::printf("ok\n");
  return 0;
}
