// Text tiles: the classify, scan and locate passes that the text parsers share (etl.hip: jsonl, submit.hip: the
// submission csv). A piece of a file (whole lines, n_bytes < 2^31, 16-byte aligned) is cut into 1024-byte tiles:
//   k_jsonl_marks<.., false> : every lane loads 16 B; a wave classifies its tile into line ends ('\n') and marks
//                              (KIND 0: a '{' that does not open its line; KIND 1: the first digit of a number) and
//                              stores one packed (lines << 32 | marks) count per tile
//   exclusive_scan_u64       : over the tile counts (no per-byte flag or index arrays)
//   k_jsonl_marks<.., true>  : the same tiling; every line start and mark goes to (tile base + rank in the tile):
//                              line_pos, line_ev (marks before the line), ev_pos, ev_line
// Each including unit instantiates its own kernels (no cross-unit device calls).
#pragma once
#include <algorithm>
#include "prims.h"
#include "table.h"

namespace ottohip {

constexpr int JSONL_TILE_BYTES = 1024;  // one wave, 16 B per lane
constexpr int JSONL_T = 256;            // threads per block: 4 tiles
static_assert(JSONL_TILE_BYTES == 64 * 16, "one 16-byte load per lane of a wave");

__device__ __forceinline__ bool is_ws(int c) { return c == ' ' || c == '\t' || c == '\r'; }
__device__ __forceinline__ bool is_digit(int c) { return c >= '0' && c <= '9'; }

// 4-bit mask of the bytes of w equal to the byte repeated in pat (bit i = byte i, lowest address first); exact
__device__ __forceinline__ uint32_t eq4(uint32_t w, uint32_t pat) {
  const uint32_t x = w ^ pat;
  uint32_t t = (x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu;
  t = ~(t | x | 0x7F7F7F7Fu);  // 0x80 in every zero byte of x
  return ((t >> 7) * 0x01020408u) >> 24;
}
__device__ __forceinline__ uint32_t eq16(const uint4& v, uint32_t pat) {
  return eq4(v.x, pat) | (eq4(v.y, pat) << 4) | (eq4(v.z, pat) << 8) | (eq4(v.w, pat) << 12);
}
__device__ __forceinline__ uint32_t byte_of(const uint4& v, int j) {
  const uint32_t w = j < 8 ? (j < 4 ? v.x : v.y) : (j < 12 ? v.z : v.w);
  return (w >> ((j & 3) * 8)) & 0xFFu;
}

// The 16 bytes at o of one lane -> (nl, mk): bit j of nl = a '\n' at o + j that is followed by another line's
// bytes, bit j of mk = a mark at o + j. Wave-uniform call (one cross-lane move).
template <int KIND>
__device__ __forceinline__ void lane_masks(const uint8_t* __restrict__ text, uint32_t n, uint32_t o, uint32_t& nl,
                                           uint32_t& mk) {
  uint4 v = make_uint4(0, 0, 0, 0);
  if (o + 16u <= n) {
    v = *reinterpret_cast<const uint4*>(text + o);
  } else if (o < n) {  // the last, short chunk of the piece: byte by byte, nothing read at or after n
    uint32_t w[4] = {0, 0, 0, 0};
    for (uint32_t j = 0; o + j < n; ++j) w[j >> 2] |= (uint32_t)text[o + j] << ((j & 3) * 8);
    v = make_uint4(w[0], w[1], w[2], w[3]);
  }
  const uint32_t valid = o >= n ? 0u : (n - o >= 16u ? 0xFFFFu : (1u << (n - o)) - 1u);
  // the byte before this lane's chunk: the lane below has it; lane 0 reads it
  uint32_t before = lane_prev(v.w >> 24);
  if (lane_id() == 0u) before = (o > 0u && o <= n) ? text[o - 1] : '\n';
  nl = eq16(v, 0x0A0A0A0Au) & valid;
  if (n - o <= 16u && o < n) nl &= ~(1u << (n - 1u - o));  // a '\n' that ends the piece starts no line
  if constexpr (KIND == 0) {
    mk = 0u;
    uint32_t br = eq16(v, 0x7B7B7B7Bu) & valid;  // '{'
    while (br) {
      const int j = __ffs((int)br) - 1;
      br &= br - 1u;
      int prev = j > 0 ? (int)byte_of(v, j - 1) : (o + j == 0u ? (int)'\n' : (int)before);
      if (is_ws(prev)) {  // white space before the brace: look further back (spaced styles; one step as a rule)
        int64_t q = (int64_t)o + j - 2;
        while (q >= 0 && is_ws(text[q])) --q;
        prev = q < 0 ? (int)'\n' : (int)text[q];
      }
      if (prev != '\n') mk |= 1u << j;
    }
  } else {
    uint32_t dg = 0u;
#pragma unroll
    for (int j = 0; j < 16; ++j) dg |= is_digit((int)byte_of(v, j)) ? 1u << j : 0u;
    dg &= valid;
    mk = dg & ~((dg << 1) | (is_digit((int)before) && o > 0u ? 1u : 0u));
  }
}

// WRITE = false: cnt[tile] = lines << 32 | marks. WRITE = true: the positions, at the scanned bases.
template <int KIND, bool WRITE>
__global__ __launch_bounds__(JSONL_T) void k_jsonl_marks(const uint8_t* __restrict__ text, uint32_t n, int64_t n_tiles,
                                                         uint64_t* __restrict__ cnt, const uint64_t* __restrict__ base,
                                                         const uint64_t* __restrict__ tot,
                                                         uint32_t* __restrict__ line_pos, uint32_t* __restrict__ line_ev,
                                                         uint32_t* __restrict__ ev_pos, uint32_t* __restrict__ ev_line) {
  const int64_t tile = (int64_t)blockIdx.x * (JSONL_T / 64) + (threadIdx.x >> 6);
  if (tile >= n_tiles) return;  // whole waves leave
  const uint32_t l = lane_id();
  const uint32_t o = (uint32_t)(tile * JSONL_TILE_BYTES) + l * 16u;
  uint32_t nl, mk;
  lane_masks<KIND>(text, n, o, nl, mk);
  const uint32_t both = ((uint32_t)__popc(nl) << 16) | (uint32_t)__popc(mk);  // at most 1024 each
  const uint32_t incl = wave_incl_scan(both);
  if constexpr (!WRITE) {
    if (l == 63u) cnt[tile] = ((uint64_t)(incl >> 16) << 32) | (incl & 0xFFFFu);
  } else {
    const uint64_t b = base[tile];
    const uint32_t excl = incl - both;
    const uint32_t nl0 = (uint32_t)(b >> 32) + (excl >> 16), mk0 = (uint32_t)b + (excl & 0xFFFFu);
    uint32_t m = nl;
    while (m) {  // the line after this '\n'
      const int j = __ffs((int)m) - 1;
      m &= m - 1u;
      const uint32_t below = (1u << j) - 1u;
      const uint32_t li = 1u + nl0 + (uint32_t)__popc(nl & below);
      line_pos[li] = o + j + 1u;
      line_ev[li] = mk0 + (uint32_t)__popc(mk & below);
    }
    if (ev_pos) {
      m = mk;
      while (m) {
        const int j = __ffs((int)m) - 1;
        m &= m - 1u;
        const uint32_t below = (1u << j) - 1u;
        const uint32_t ei = mk0 + (uint32_t)__popc(mk & below);
        ev_pos[ei] = o + j;
        ev_line[ei] = nl0 + (uint32_t)__popc(nl & below);
      }
    }
    if (tile == 0 && l == 0u) {  // the first line, and the closing entries
      const uint64_t t = *tot;
      const uint32_t n_lines = (uint32_t)(t >> 32) + 1u;
      line_pos[0] = 0u;
      line_ev[0] = 0u;
      line_pos[n_lines] = n;
      line_ev[n_lines] = (uint32_t)t;
    }
  }
}

// ---------------------------------------------------------------- host side
struct JsonlScan {
  int64_t n_tiles = 0, n_lines = 0, n_marks = 0;
  uint64_t *cnt = nullptr, *base = nullptr, *tot = nullptr;
  uint32_t *line_pos = nullptr, *line_ev = nullptr, *ev_pos = nullptr, *ev_line = nullptr;
};

static int jsonl_args(const char* who, ottohip_ctx* c, const uint8_t* text, int64_t n_bytes) {
  if (!c || n_bytes < 0 || (n_bytes > 0 && !text)) { set_error("%s: bad arguments", who); return OTTOHIP_EINVAL; }
  if (n_bytes >= ((int64_t)1 << 31)) { set_error("%s: a piece of %lld bytes >= 2^31", who, (long long)n_bytes); return OTTOHIP_ELIMIT; }
  if (reinterpret_cast<uintptr_t>(text) & 15u) { set_error("%s: text is not 16-byte aligned", who); return OTTOHIP_EINVAL; }
  return 0;
}

template <int KIND>
static int jsonl_count(Ctx* ctx, const uint8_t* text, int64_t n, JsonlScan& J, hipStream_t s) {
  Workspace& ws = ctx->ws;
  J.n_tiles = ceil_div(n, JSONL_TILE_BYTES);
  OH_TRY(ws.get("jl_cnt", (size_t)J.n_tiles, &J.cnt));
  OH_TRY(ws.get("jl_base", (size_t)J.n_tiles, &J.base));
  OH_TRY(ws.get("jl_tot", 1, &J.tot));
  int ph = ctx->begin("jsonl_classify", s, (double)n + 8.0 * (double)J.n_tiles);
  k_jsonl_marks<KIND, false><<<grid_for(J.n_tiles, JSONL_T / 64), JSONL_T, 0, s>>>(
      text, (uint32_t)n, J.n_tiles, J.cnt, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  OH_HIP(hipGetLastError());
  ctx->end(ph, s);
  ph = ctx->begin("jsonl_scan", s, 16.0 * (double)J.n_tiles);
  OH_TRY(exclusive_scan_u64(ctx, J.cnt, J.base, J.n_tiles, J.tot, s));
  ctx->end(ph, s);
  uint64_t t = 0;
  OH_TRY(d2h(&t, J.tot, 1, s));
  J.n_lines = (int64_t)(t >> 32) + 1;
  J.n_marks = (int64_t)(t & 0xFFFFFFFFu);
  return 0;
}

// marks: also the position and the line of every mark (ev_pos, ev_line)
template <int KIND>
static int jsonl_locate(Ctx* ctx, const uint8_t* text, int64_t n, JsonlScan& J, hipStream_t s, bool marks = KIND == 0) {
  Workspace& ws = ctx->ws;
  OH_TRY(ws.get("jl_line_pos", (size_t)J.n_lines + 1, &J.line_pos));
  OH_TRY(ws.get("jl_line_ev", (size_t)J.n_lines + 1, &J.line_ev));
  if (marks) {
    OH_TRY(ws.get("jl_ev_pos", (size_t)std::max<int64_t>(J.n_marks, 1), &J.ev_pos));
    OH_TRY(ws.get("jl_ev_line", (size_t)std::max<int64_t>(J.n_marks, 1), &J.ev_line));
  }
  const int ph = ctx->begin("jsonl_locate", s, (double)n + 8.0 * (double)(J.n_tiles + J.n_lines + (marks ? J.n_marks : 0)));
  k_jsonl_marks<KIND, true><<<grid_for(J.n_tiles, JSONL_T / 64), JSONL_T, 0, s>>>(
      text, (uint32_t)n, J.n_tiles, nullptr, J.base, J.tot, J.line_pos, J.line_ev, J.ev_pos, J.ev_line);
  OH_HIP(hipGetLastError());
  ctx->end(ph, s);
  return 0;
}

}  // namespace ottohip
