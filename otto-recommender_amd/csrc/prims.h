#pragma once
#include "common.h"

namespace ottohip {
// out[i] = sum(in[0..i)), 64-bit; optional device total
int exclusive_scan_u32(Ctx* ctx, const uint32_t* in, uint64_t* out, int64_t n, uint64_t* total,
                       hipStream_t s);
int exclusive_scan_u64(Ctx* ctx, const uint64_t* in, uint64_t* out, int64_t n, uint64_t* total,
                       hipStream_t s);
// stable LSD sort of (key, val) in whole 8-bit passes from bit shift0 up to bits, rounded up to a byte: the result
// is the stable order by key bits [shift0, 8 * ceil(bits / 8)); key bits at or above that are carried unchanged and
// do not order anything (the co-visitation rows carry a count above a byte-aligned key). Ping-pongs with the *_alt
// buffers and returns the buffers holding the result in keys/vals
// iota_vals: the input values are their own indices (0..n-1); the first pass generates them
// instead of reading vals (vals still provides the buffer)
// skip (with iota_vals): the first pass drops keys with (key & mask) == inv and the later passes sort the
// *n_out kept pairs (the first pass' total, read back on the host).
// inv must lie inside mask, (inv & ~mask) == 0: the passes pad their last tile with inv and rely on the padding
// being dropped. radix_skip_pass, and radix_sort_pairs with skip, return OTTOHIP_EINVAL for any other pair and
// launch nothing
struct SortSkip {
  uint32_t mask, inv;
  int64_t* n_out;
};
// shift0 (a multiple of 8, without skip): the passes start at this bit; the input must already be ordered by the
// key bits [0, shift0), and the result is then ordered by the bits [0, 8 * ceil(bits / 8))
int radix_sort_pairs(Ctx* ctx, uint32_t*& keys, uint32_t*& vals, uint32_t* keys_alt, uint32_t* vals_alt,
                     int64_t n, int bits, hipStream_t s, bool iota_vals = false, const SortSkip* skip = nullptr,
                     int shift0 = 0);
// the compacting first pass alone: keys[0, n) -> (kout, vout), the kept (key, index) pairs bucketed by key & 255 in
// index order; *skip.n_out = the kept count (read back on the host). digit_start / n_tiles as in radix_pass: bucket d
// starts at (*digit_start)[d * *n_tiles], valid until the next radix pass on ctx.
// radix_sort_pairs(kout, vout, ..., shift0 = 8) over the kept pairs finishes the sort.
int radix_skip_pass(Ctx* ctx, const uint32_t* keys, uint32_t* kout, uint32_t* vout, int64_t n, hipStream_t s,
                    const SortSkip& skip, const uint64_t** digit_start = nullptr, int* n_tiles = nullptr);
// keys per tile of a radix pass: column t of digit_start covers the input keys [t, t + 1) * RADIX_TILE_KEYS
#ifndef OH_RS_R
#define OH_RS_R 16  // keys per thread and sub-tile (A/B build flag)
#endif
constexpr int RADIX_TILE_KEYS = 256 * OH_RS_R * 4;
// one stable 8-bit pass on digit (key >> shift) & 255
int radix_pass(Ctx* ctx, const uint32_t* kin, const uint32_t* vin, uint32_t* kout, uint32_t* vout, int64_t n,
               int shift, hipStream_t s, const uint64_t** digit_start = nullptr, int* n_tiles = nullptr);
}  // namespace ottohip
