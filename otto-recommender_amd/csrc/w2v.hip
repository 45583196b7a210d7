// Word2Vec item embeddings: synchronous mini-batch CBOW with negative sampling (DESIGN.md "Word2Vec trainer").
//
//   compaction   per epoch: an event is kept when its type is in the mask, its aid has a vocabulary row and its keep
//                draw passes the row's threshold; the kept events of a session, in order, are one sentence
//   batch        one wave per kept position: lane l holds dims l and l + 64 of every vector. The context rows are
//                summed in position order, every target's dot is a two-product partial per lane folded by an xor
//                butterfly over 32..1, and every update is rounded to int64 fixed point (2^shift) and added with
//                no-return 64-bit integer atomics, 64 consecutive dims per instruction: the sums do not depend on the
//                order of arrival, so two fits give the same bytes. All positions of a batch read the weights as they
//                stood at its start.
//   apply        rows whose touched flag is set: w += (float)((double)acc * 2^-shift), acc = 0, flag = 0
//
// The unit is compiled with -ffp-contract=off: tests/w2v_oracle.py restates every fp32 operation in numpy in the same
// order, and a * b + c must stay two roundings. Nothing here calls expf: the sigmoid is a host-built table. The rate
// of 64-bit integer atomics on gfx950 is not measured anywhere in this project; tools/w2v_timing.py records what the
// batch kernel reaches.
#include "prims.h"
#include "table.h"

#include <algorithm>
#include <cmath>

namespace ottohip {

constexpr int W2V_T = 256;             // threads per block: 4 waves, one position each
constexpr int W2V_MAX_DIM = 128;       // two dims per lane
constexpr int W2V_MAX_WINDOW = 31;     // the 2 * window + 1 rows of a window sit one per lane
constexpr int W2V_MAX_NEGATIVE = 32;   // one draw per lane

__host__ __device__ __forceinline__ uint64_t w2v_mix(uint64_t z) {  // the draw of downsample.hip
  z += 0x9E3779B97F4A7C15ull;
  z ^= z >> 30;
  z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27;
  z *= 0x94D049BB133111EBull;
  z ^= z >> 31;
  return z;
}
// seed_mix = w2v_mix(seed); slot 0: keep, 1: reduced window, 2 + j: negative j; index: the event's place in the CSR
__host__ __device__ __forceinline__ uint64_t w2v_draw(uint64_t seed_mix, uint32_t epoch, uint32_t slot, uint32_t index) {
  return w2v_mix(w2v_mix(seed_mix ^ (((uint64_t)epoch << 32) | (uint64_t)slot)) ^ (uint64_t)index);
}

// session of every event: the last s with off[s] <= i
__global__ __launch_bounds__(W2V_T) void k_w2v_sid(const int64_t* __restrict__ off, int64_t n_sessions, int64_t n,
                                                    int32_t* __restrict__ sid) {
  for (int64_t i = (int64_t)blockIdx.x * W2V_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * W2V_T) {
    int64_t lo = 0, hi = n_sessions;  // first s in [0, n_sessions] with off[s] > i
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (off[mid] > i) hi = mid; else lo = mid + 1;
    }
    sid[i] = (int32_t)(lo > 0 ? lo - 1 : 0);
  }
}

__device__ __forceinline__ int32_t w2v_row_of(const int32_t* __restrict__ row_of_aid, int32_t n_items, int64_t V,
                                              int32_t aid) {
  if (aid < 0 || aid >= n_items) return -1;
  const int32_t r = row_of_aid[aid];
  return (r >= 0 && (int64_t)r < V) ? r : -1;
}

__global__ __launch_bounds__(W2V_T) void k_w2v_keep(const int32_t* __restrict__ aid, const int8_t* __restrict__ type,
                                                     int64_t n, const int32_t* __restrict__ row_of_aid, int32_t n_items,
                                                     const uint32_t* __restrict__ keep_thr, int64_t V, uint32_t type_mask,
                                                     uint64_t seed_mix, uint32_t epoch, uint32_t* __restrict__ keep) {
  for (int64_t i = (int64_t)blockIdx.x * W2V_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * W2V_T) {
    const int ty = (int)type[i];
    uint32_t k = 0;
    if (ty >= 0 && ty < 32 && ((type_mask >> ty) & 1u)) {
      const int32_t r = w2v_row_of(row_of_aid, n_items, V, aid[i]);
      if (r >= 0) k = (uint32_t)(w2v_draw(seed_mix, epoch, 0u, (uint32_t)i) >> 32) <= keep_thr[r] ? 1u : 0u;
    }
    keep[i] = k;
  }
}

__global__ __launch_bounds__(W2V_T) void k_w2v_scatter(const int32_t* __restrict__ aid, int64_t n,
                                                        const int32_t* __restrict__ row_of_aid, int32_t n_items, int64_t V,
                                                        const uint32_t* __restrict__ keep, const uint64_t* __restrict__ pos,
                                                        const int32_t* __restrict__ sid, int32_t* __restrict__ rows,
                                                        int32_t* __restrict__ orig, int32_t* __restrict__ csid) {
  for (int64_t i = (int64_t)blockIdx.x * W2V_T + threadIdx.x; i < n; i += (int64_t)gridDim.x * W2V_T) {
    if (!keep[i]) continue;
    const uint64_t p = pos[i];  // < n: the kept events before i
    rows[p] = w2v_row_of(row_of_aid, n_items, V, aid[i]);
    orig[p] = (int32_t)i;
    csid[p] = sid[i];
  }
}

// sentence offsets: the kept events before each session's first event; coff[n_sessions] = the kept count
__global__ __launch_bounds__(W2V_T) void k_w2v_coff(const int64_t* __restrict__ off, int64_t n_sessions, int64_t n,
                                                     const uint64_t* __restrict__ pos, const uint64_t* __restrict__ total,
                                                     int64_t* __restrict__ coff) {
  for (int64_t s = (int64_t)blockIdx.x * W2V_T + threadIdx.x; s <= n_sessions; s += (int64_t)gridDim.x * W2V_T) {
    const int64_t o = off[s];  // off[0] == 0
    coff[s] = (s == n_sessions || o >= n) ? (int64_t)*total : (int64_t)pos[o < 0 ? 0 : o];
  }
}

__device__ __forceinline__ float w2v_wave_sum(float v) {  // xor butterfly 32, 16, 8, 4, 2, 1: every lane gets the sum
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
  return v;
}

__device__ __forceinline__ long long w2v_fixed(float x, double scale, double clamp) {
  double v = rint((double)x * scale);
  if (!(v == v)) v = 0.0;  // NaN adds nothing
  v = fmin(fmax(v, -clamp), clamp);
  return (long long)v;
}

struct W2vBatch {
  const int32_t* rows;     // [n_kept] vocabulary row per kept position
  const int32_t* orig;     // [n_kept] the event's index (the key of its draws)
  const int32_t* csid;     // [n_kept] sentence of the position
  const int64_t* coff;     // [n_sessions + 1] sentence offsets
  int64_t n_kept, n_sessions, b0, b1;
  const float* syn0;       // [V][dim]
  const float* syn1;       // [V][dim]
  int64_t V;
  int dim, window, negative;
  const uint32_t* cum;     // [V] 31-bit cumulative negative table
  const float* sig;        // [n_sig] sigmoid over [-max_exp, max_exp)
  int n_sig;
  float max_exp, sig_scale, lr;
  uint64_t seed_mix;
  uint32_t epoch;
  double scale, clamp;
  long long* acc0;         // [V][dim]
  long long* acc1;
  uint8_t* flag0;          // [V]
  uint8_t* flag1;
};

__global__ __launch_bounds__(W2V_T) void k_w2v_batch(const W2vBatch B) {
  const int l = (int)lane_id();
  const int64_t p = B.b0 + (int64_t)blockIdx.x * (W2V_T / 64) +
                    (int64_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (p >= B.b1) return;
  const int32_t w = B.rows[p];
  const int32_t sd = B.csid[p];
  if (w < 0 || (int64_t)w >= B.V || sd < 0 || (int64_t)sd >= B.n_sessions) return;
  const uint32_t oi = (uint32_t)B.orig[p];
  // lane 0: the reduced-window draw; lanes 1..negative: the negatives, each by its own search of the table
  uint32_t mine = 0;
  if (l <= B.negative) {
    const uint64_t d = w2v_draw(B.seed_mix, B.epoch, (uint32_t)(l + 1), oi);
    if (l == 0) {
      mine = (uint32_t)(d % (uint64_t)B.window);
    } else {
      const uint32_t x = (uint32_t)(d >> 33);
      int64_t lo = 0, hi = B.V;  // first row with cum > x
      while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (B.cum[mid] > x) hi = mid; else lo = mid + 1;
      }
      mine = (uint32_t)(lo < B.V ? lo : B.V - 1);
    }
  }
  const int eff = B.window - (int)__shfl((int)mine, 0);
  // the window inside the sentence; the further bounds keep every index inside the arrays whatever the caller gave
  int64_t lo = B.coff[sd], hi = B.coff[sd + 1] - 1;
  if (lo < p - eff) lo = p - eff;
  if (hi > p + eff) hi = p + eff;
  if (lo < 0) lo = 0;
  if (hi > B.n_kept - 1) hi = B.n_kept - 1;
  if (lo > p) lo = p;
  if (hi < p) hi = p;
  const int n_win = (int)(hi - lo + 1);  // <= 2 * window + 1 <= 63
  const int self = (int)(p - lo);
  const int cnt = n_win - 1;
  if (cnt <= 0) return;
  // the window's rows, one per lane; a row outside the vocabulary drops the position
  const int32_t wr = l < n_win ? B.rows[lo + l] : 0;
  if (__ballot(wr < 0 || (int64_t)wr >= B.V)) return;

  const int dim = B.dim;
  const bool in0 = l < dim, in1 = l + 64 < dim;
  float a0 = 0.0f, a1 = 0.0f;
  for (int c = 0; c < n_win; ++c) {
    if (c == self) continue;
    const float* r = B.syn0 + (int64_t)__shfl(wr, c) * dim;
    a0 = a0 + (in0 ? r[l] : 0.0f);
    a1 = a1 + (in1 ? r[l + 64] : 0.0f);
  }
  const float fc = (float)cnt;
  const float h0 = a0 / fc, h1 = a1 / fc;
  float e0 = 0.0f, e1 = 0.0f;
  for (int t = 0; t <= B.negative; ++t) {
    const int32_t tr = t == 0 ? w : (int32_t)__shfl((int)mine, t);
    if (t > 0 && tr == w) continue;
    const float* r = B.syn1 + (int64_t)tr * dim;
    const float s0 = in0 ? r[l] : 0.0f, s1 = in1 ? r[l + 64] : 0.0f;
    const float f = w2v_wave_sum(h0 * s0 + h1 * s1);
    if (!(f > -B.max_exp && f < B.max_exp)) continue;
    int idx = (int)((f + B.max_exp) * B.sig_scale);
    idx = idx < 0 ? 0 : (idx > B.n_sig - 1 ? B.n_sig - 1 : idx);
    const float g = ((t == 0 ? 1.0f : 0.0f) - B.sig[idx]) * B.lr;
    e0 = e0 + g * s0;
    e1 = e1 + g * s1;
    unsigned long long* a = reinterpret_cast<unsigned long long*>(B.acc1) + (int64_t)tr * dim;
    if (in0) atomicAdd(a + l, (unsigned long long)w2v_fixed(g * h0, B.scale, B.clamp));
    if (in1) atomicAdd(a + l + 64, (unsigned long long)w2v_fixed(g * h1, B.scale, B.clamp));
    if (l == 0) B.flag1[tr] = 1;
  }
  const unsigned long long v0 = (unsigned long long)w2v_fixed(e0, B.scale, B.clamp);
  const unsigned long long v1 = (unsigned long long)w2v_fixed(e1, B.scale, B.clamp);
  for (int c = 0; c < n_win; ++c) {
    if (c == self) continue;
    const int32_t cr = __shfl(wr, c);
    unsigned long long* a = reinterpret_cast<unsigned long long*>(B.acc0) + (int64_t)cr * dim;
    if (in0) atomicAdd(a + l, v0);
    if (in1) atomicAdd(a + l + 64, v1);
    if (l == 0) B.flag0[cr] = 1;
  }
}

// one wave per 64 rows: the flags by lane, then the flagged rows one after another, two dims per lane
__global__ __launch_bounds__(W2V_T) void k_w2v_apply(float* __restrict__ w, long long* __restrict__ acc,
                                                      uint8_t* __restrict__ flag, int64_t V, int dim, double inv_scale) {
  const int l = (int)lane_id();
  const int64_t n_chunks = ceil_div(V, 64);
  const int64_t wave0 = (int64_t)blockIdx.x * (W2V_T / 64) + (threadIdx.x >> 6);
  for (int64_t ch = wave0; ch < n_chunks; ch += (int64_t)gridDim.x * (W2V_T / 64)) {
    const int64_t r_l = ch * 64 + l;
    const bool on = r_l < V && flag[r_l] != 0;
    uint64_t m = __ballot(on);
    if (on) flag[r_l] = 0;
    while (m) {
      const int b = __ffsll((long long)m) - 1;
      m &= m - 1;
      const int64_t base = (ch * 64 + b) * dim;
      for (int d = l; d < dim; d += 64) {
        w[base + d] = w[base + d] + (float)((double)acc[base + d] * inv_scale);
        acc[base + d] = 0;
      }
    }
  }
}

struct W2vCompactBufs {
  int32_t *sid, *rows, *orig, *csid;
  uint32_t* keep;
  uint64_t *pos, *total;
  int64_t* coff;
};

// one epoch's compaction; *n_kept through one host read
static int w2v_compact(ottohip_ctx* ctx, const int64_t* off, int64_t n_sessions, const int32_t* aid, const int8_t* type,
                       int64_t n, const int32_t* row_of_aid, int32_t n_items, const uint32_t* keep_thr, int64_t V,
                       uint32_t type_mask, uint64_t seed, uint32_t epoch, const W2vCompactBufs& C, bool have_sid,
                       int64_t* n_kept, hipStream_t s) {
  const unsigned grid_e = (unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div(n, W2V_T), 1), (int64_t)ctx->n_cu * 16);
  const unsigned grid_s =
      (unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div(n_sessions + 1, W2V_T), 1), (int64_t)ctx->n_cu * 16);
  OH_HIP(hipMemsetAsync(C.total, 0, sizeof(uint64_t), s));
  if (n > 0) {
    if (!have_sid) k_w2v_sid<<<grid_e, W2V_T, 0, s>>>(off, n_sessions, n, C.sid);
    k_w2v_keep<<<grid_e, W2V_T, 0, s>>>(aid, type, n, row_of_aid, n_items, keep_thr, V, type_mask, w2v_mix(seed), epoch,
                                        C.keep);
    OH_HIP(hipGetLastError());
    OH_TRY(exclusive_scan_u32(ctx, C.keep, C.pos, n, C.total, s));
    k_w2v_scatter<<<grid_e, W2V_T, 0, s>>>(aid, n, row_of_aid, n_items, V, C.keep, C.pos, C.sid, C.rows, C.orig, C.csid);
  }
  k_w2v_coff<<<grid_s, W2V_T, 0, s>>>(off, n_sessions, n, C.pos, C.total, C.coff);
  OH_HIP(hipGetLastError());
  uint64_t tot = 0;
  OH_TRY(d2h(&tot, C.total, 1, s));
  *n_kept = (int64_t)tot;
  return 0;
}

static int w2v_check_params(const ottohip_w2v_params* P, const char* who) {
  if (!P || P->dim < 1 || P->dim > W2V_MAX_DIM || P->window < 1 || P->window > W2V_MAX_WINDOW || P->negative < 0 ||
      P->negative > W2V_MAX_NEGATIVE || P->n_sig < 1 || !(P->max_exp > 0.0) || P->shift < 1 || P->shift > 48 ||
      P->batch_positions < 1 || P->batch_positions > ((int64_t)1 << 30) || P->epochs < 1) {
    set_error("%s: bad parameters (1 <= dim <= %d, 1 <= window <= %d, 0 <= negative <= %d, n_sig >= 1, max_exp > 0, "
              "1 <= shift <= 48, 1 <= batch_positions <= 2^30, epochs >= 1)",
              who, W2V_MAX_DIM, W2V_MAX_WINDOW, W2V_MAX_NEGATIVE);
    return OTTOHIP_EINVAL;
  }
  return 0;
}

// the largest |contribution|: a power of two C with (most contributions to one row in a batch) * C <= 2^62
static double w2v_clamp(const ottohip_w2v_params& P) {
  const int64_t per_pos = std::max<int64_t>(1 + P.negative, 2 * (int64_t)P.window);
  return std::ldexp(1.0, 62 - bits_for((uint64_t)(P.batch_positions * per_pos)));
}

static W2vBatch w2v_batch_args(const ottohip_w2v_params& P, const int32_t* rows, const int32_t* orig, const int32_t* csid,
                               const int64_t* coff, int64_t n_kept, int64_t n_sessions, int64_t b0, int64_t b1,
                               const float* syn0, const float* syn1, int64_t V, const uint32_t* cum, const float* sig,
                               uint32_t epoch, float lr, long long* acc0, long long* acc1, uint8_t* flag0,
                               uint8_t* flag1) {
  W2vBatch B;
  B.rows = rows; B.orig = orig; B.csid = csid; B.coff = coff;
  B.n_kept = n_kept; B.n_sessions = n_sessions; B.b0 = b0; B.b1 = b1;
  B.syn0 = syn0; B.syn1 = syn1; B.V = V;
  B.dim = P.dim; B.window = P.window; B.negative = P.negative;
  B.cum = cum; B.sig = sig; B.n_sig = P.n_sig;
  B.max_exp = (float)P.max_exp;
  B.sig_scale = (float)((double)P.n_sig / (2.0 * P.max_exp));
  B.lr = lr;
  B.seed_mix = w2v_mix(P.seed);
  B.epoch = epoch;
  B.scale = std::ldexp(1.0, P.shift);
  B.clamp = w2v_clamp(P);
  B.acc0 = acc0; B.acc1 = acc1; B.flag0 = flag0; B.flag1 = flag1;
  return B;
}

static unsigned w2v_apply_grid(const ottohip_ctx* ctx, int64_t V) {
  return (unsigned)std::min<int64_t>(std::max<int64_t>(ceil_div(ceil_div(V, 64), W2V_T / 64), 1), (int64_t)ctx->n_cu * 8);
}

template <class T>
static int w2v_alloc(T** p, size_t n, const char* what) {
  hipError_t e = dev_alloc(reinterpret_cast<void**>(p), std::max<size_t>(n, 1) * sizeof(T), what);
  if (e != hipSuccess) {
    set_error("w2v: allocation of %s failed: %s", what, hipGetErrorString(e));
    return OTTOHIP_ENOMEM;
  }
  return 0;
}

}  // namespace ottohip

using namespace ottohip;

struct ottohip_w2v {
  ottohip_ctx* ctx = nullptr;
  ottohip_events ev{};
  const int32_t* row_of_aid = nullptr;
  int32_t n_items = 0;
  const uint32_t *keep_thr = nullptr, *cum = nullptr;
  const float* sig = nullptr;
  int64_t V = 0;
  ottohip_w2v_params P{};
  float *syn0 = nullptr, *syn1 = nullptr;
  long long *acc0 = nullptr, *acc1 = nullptr;
  uint8_t *flag0 = nullptr, *flag1 = nullptr;
  W2vCompactBufs C{};
  bool have_sid = false;
};

extern "C" {

int ottohip_w2v_compact(ottohip_ctx* ctx, const ottohip_events* ev, const int32_t* row_of_aid, int32_t n_items,
                        const uint32_t* keep_thr, int64_t n_vocab, uint32_t type_mask, uint64_t seed, int32_t epoch,
                        int32_t* rows, int32_t* orig, int32_t* sid, int64_t* offsets, int64_t* n_kept, void* stream) {
  if (!ctx || !ev || !n_kept || !offsets || ev->n_events < 0 || ev->n_events >= ((int64_t)1 << 31) ||
      ev->n_sessions < 0 || ev->n_sessions >= ((int64_t)1 << 31) || !ev->session_offsets || n_items < 0 || n_vocab < 0 ||
      epoch < 0 || (n_items > 0 && !row_of_aid) || (n_vocab > 0 && !keep_thr) ||
      (ev->n_events > 0 && (!ev->aid || !ev->type || !rows || !orig || !sid))) {
    set_error("w2v_compact: bad arguments (events and sessions below 2^31, outputs not NULL)");
    return OTTOHIP_EINVAL;
  }
  OH_HIP(hipSetDevice(ctx->device));
  hipStream_t s = S(stream);
  const size_t n = (size_t)ev->n_events;
  W2vCompactBufs C{};
  OH_TRY(ctx->ws.get("w2v_sid", std::max<size_t>(n, 1), &C.sid));
  OH_TRY(ctx->ws.get("w2v_keep", std::max<size_t>(n, 1), &C.keep));
  OH_TRY(ctx->ws.get("w2v_pos", std::max<size_t>(n, 1), &C.pos));
  OH_TRY(ctx->ws.get("w2v_total", 1, &C.total));
  C.rows = rows; C.orig = orig; C.csid = sid; C.coff = offsets;
  return w2v_compact(ctx, ev->session_offsets, ev->n_sessions, ev->aid, ev->type, ev->n_events, row_of_aid, n_items,
                     keep_thr, n_vocab, type_mask, seed, (uint32_t)epoch, C, false, n_kept, s);
}

int ottohip_w2v_batch(ottohip_ctx* ctx, const int32_t* rows, const int32_t* orig, const int32_t* sid,
                      const int64_t* offsets, int64_t n_kept, int64_t n_sessions, int64_t b0, int64_t b1,
                      const float* syn0, const float* syn1neg, int64_t n_vocab, const uint32_t* cum, const float* sig,
                      const ottohip_w2v_params* params, int32_t epoch, float lr, long long* acc0, long long* acc1,
                      uint8_t* flag0, uint8_t* flag1, void* stream) {
  OH_TRY(w2v_check_params(params, "w2v_batch"));
  if (!ctx || n_kept < 0 || n_sessions < 0 || b0 < 0 || b1 < b0 || b1 > n_kept || b1 - b0 > params->batch_positions ||
      n_vocab < 1 || n_vocab >= ((int64_t)1 << 31) || epoch < 0 || !rows || !orig || !sid || !offsets || !syn0 ||
      !syn1neg || !cum || !sig || !acc0 || !acc1 || !flag0 || !flag1) {
    set_error("w2v_batch: bad arguments (0 <= b0 <= b1 <= n_kept, b1 - b0 <= batch_positions, 1 <= n_vocab < 2^31, "
              "arrays not NULL)");
    return OTTOHIP_EINVAL;
  }
  if (b1 == b0) return 0;
  OH_HIP(hipSetDevice(ctx->device));
  const W2vBatch B = w2v_batch_args(*params, rows, orig, sid, offsets, n_kept, n_sessions, b0, b1, syn0, syn1neg, n_vocab,
                                    cum, sig, (uint32_t)epoch, lr, acc0, acc1, flag0, flag1);
  k_w2v_batch<<<(unsigned)ceil_div(b1 - b0, W2V_T / 64), W2V_T, 0, S(stream)>>>(B);
  OH_HIP(hipGetLastError());
  return 0;
}

int ottohip_w2v_apply(ottohip_ctx* ctx, float* weights, long long* acc, uint8_t* flag, int64_t n_vocab, int dim,
                      int shift, void* stream) {
  if (!ctx || n_vocab < 0 || dim < 1 || dim > W2V_MAX_DIM || shift < 1 || shift > 48 ||
      (n_vocab > 0 && (!weights || !acc || !flag))) {
    set_error("w2v_apply: bad arguments (1 <= dim <= %d, 1 <= shift <= 48)", W2V_MAX_DIM);
    return OTTOHIP_EINVAL;
  }
  if (n_vocab == 0) return 0;
  OH_HIP(hipSetDevice(ctx->device));
  k_w2v_apply<<<w2v_apply_grid(ctx, n_vocab), W2V_T, 0, S(stream)>>>(weights, acc, flag, n_vocab, dim,
                                                                     std::ldexp(1.0, -shift));
  OH_HIP(hipGetLastError());
  return 0;
}

void ottohip_w2v_free(ottohip_w2v* t) {
  if (!t) return;
  (void)hipDeviceSynchronize();
  void* bufs[] = {t->syn0, t->syn1, t->acc0, t->acc1, t->flag0, t->flag1, t->C.sid, t->C.rows, t->C.orig, t->C.csid,
                  t->C.keep, t->C.pos, t->C.total, t->C.coff};
  for (void* p : bufs)
    if (p) dev_free(p);
  delete t;
}

int ottohip_w2v_create(ottohip_ctx* ctx, const ottohip_events* ev, const int32_t* row_of_aid, int32_t n_items,
                       const uint32_t* keep_thr, const uint32_t* cum, int64_t n_vocab, const float* sig,
                       const float* syn0_init, const ottohip_w2v_params* params, ottohip_w2v** out) {
  OH_TRY(w2v_check_params(params, "w2v_create"));
  if (!ctx || !out || !ev || ev->n_events < 0 || ev->n_events >= ((int64_t)1 << 31) || ev->n_sessions < 0 ||
      ev->n_sessions >= ((int64_t)1 << 31) || !ev->session_offsets || (ev->n_events > 0 && (!ev->aid || !ev->type)) ||
      n_items < 0 || (n_items > 0 && !row_of_aid) || n_vocab < 1 || n_vocab >= ((int64_t)1 << 31) || !keep_thr || !cum ||
      !sig || !syn0_init) {
    set_error("w2v_create: bad arguments (events and sessions below 2^31, 1 <= n_vocab < 2^31, arrays not NULL)");
    return OTTOHIP_EINVAL;
  }
  *out = nullptr;
  OH_HIP(hipSetDevice(ctx->device));
  ottohip_w2v* t = new ottohip_w2v();
  t->ctx = ctx; t->ev = *ev; t->row_of_aid = row_of_aid; t->n_items = n_items; t->keep_thr = keep_thr; t->cum = cum;
  t->sig = sig; t->V = n_vocab; t->P = *params;
  const size_t n = (size_t)ev->n_events, vd = (size_t)n_vocab * (size_t)params->dim;
  int rc = 0;
  if ((rc = w2v_alloc(&t->syn0, vd, "syn0")) || (rc = w2v_alloc(&t->syn1, vd, "syn1neg")) ||
      (rc = w2v_alloc(&t->acc0, vd, "syn0 sums")) || (rc = w2v_alloc(&t->acc1, vd, "syn1neg sums")) ||
      (rc = w2v_alloc(&t->flag0, (size_t)n_vocab, "syn0 flags")) ||
      (rc = w2v_alloc(&t->flag1, (size_t)n_vocab, "syn1neg flags")) || (rc = w2v_alloc(&t->C.sid, n, "sessions")) ||
      (rc = w2v_alloc(&t->C.rows, n, "rows")) || (rc = w2v_alloc(&t->C.orig, n, "events")) ||
      (rc = w2v_alloc(&t->C.csid, n, "sentences")) || (rc = w2v_alloc(&t->C.keep, n, "keep")) ||
      (rc = w2v_alloc(&t->C.pos, n, "positions")) || (rc = w2v_alloc(&t->C.total, 1, "kept")) ||
      (rc = w2v_alloc(&t->C.coff, (size_t)ev->n_sessions + 1, "sentence offsets"))) {
    ottohip_w2v_free(t);
    return rc;
  }
  if (hipMemcpy(t->syn0, syn0_init, vd * sizeof(float), hipMemcpyDeviceToDevice) != hipSuccess ||
      hipMemset(t->syn1, 0, vd * sizeof(float)) != hipSuccess ||
      hipMemset(t->acc0, 0, vd * sizeof(long long)) != hipSuccess ||
      hipMemset(t->acc1, 0, vd * sizeof(long long)) != hipSuccess ||
      hipMemset(t->flag0, 0, (size_t)n_vocab) != hipSuccess || hipMemset(t->flag1, 0, (size_t)n_vocab) != hipSuccess) {
    ottohip_w2v_free(t);
    set_error("w2v_create: initialising the weights failed");
    return OTTOHIP_EHIP;
  }
  *out = t;
  return 0;
}

int ottohip_w2v_epoch(ottohip_w2v* t, int32_t epoch, int64_t* n_kept, int64_t* n_batches, void* stream) {
  if (!t || epoch < 0 || epoch >= t->P.epochs) {
    set_error("w2v_epoch: bad arguments (0 <= epoch < epochs)");
    return OTTOHIP_EINVAL;
  }
  OH_HIP(hipSetDevice(t->ctx->device));
  hipStream_t s = S(stream);
  const ottohip_w2v_params& P = t->P;
  int64_t N = 0;
  OH_TRY(w2v_compact(t->ctx, t->ev.session_offsets, t->ev.n_sessions, t->ev.aid, t->ev.type, t->ev.n_events,
                     t->row_of_aid, t->n_items, t->keep_thr, t->V, P.type_mask, P.seed, (uint32_t)epoch, t->C,
                     t->have_sid, &N, s));
  t->have_sid = true;
  const int64_t Bp = P.batch_positions, nb = ceil_div(N, Bp);
  const unsigned ag = w2v_apply_grid(t->ctx, t->V);
  const double inv = std::ldexp(1.0, -P.shift);
  for (int64_t b = 0; b < nb; ++b) {
    double a = P.alpha - (P.alpha - P.min_alpha) * (((double)epoch + (double)(b * Bp) / (double)N) / (double)P.epochs);
    if (a < P.min_alpha) a = P.min_alpha;
    const int64_t b0 = b * Bp, b1 = std::min(N, b0 + Bp);
    const W2vBatch B = w2v_batch_args(P, t->C.rows, t->C.orig, t->C.csid, t->C.coff, N, t->ev.n_sessions, b0, b1, t->syn0,
                                      t->syn1, t->V, t->cum, t->sig, (uint32_t)epoch, (float)a, t->acc0, t->acc1,
                                      t->flag0, t->flag1);
    k_w2v_batch<<<(unsigned)ceil_div(b1 - b0, W2V_T / 64), W2V_T, 0, s>>>(B);
    k_w2v_apply<<<ag, W2V_T, 0, s>>>(t->syn0, t->acc0, t->flag0, t->V, P.dim, inv);
    k_w2v_apply<<<ag, W2V_T, 0, s>>>(t->syn1, t->acc1, t->flag1, t->V, P.dim, inv);
  }
  OH_HIP(hipGetLastError());
  if (n_kept) *n_kept = N;
  if (n_batches) *n_batches = nb;
  return 0;
}

int ottohip_w2v_vectors(const ottohip_w2v* t, float* syn0, float* syn1neg, void* stream) {
  if (!t || !syn0) { set_error("w2v_vectors: bad arguments"); return OTTOHIP_EINVAL; }
  OH_HIP(hipSetDevice(t->ctx->device));
  const size_t bytes = (size_t)t->V * (size_t)t->P.dim * sizeof(float);
  OH_HIP(hipMemcpyAsync(syn0, t->syn0, bytes, hipMemcpyDeviceToDevice, S(stream)));
  if (syn1neg) OH_HIP(hipMemcpyAsync(syn1neg, t->syn1, bytes, hipMemcpyDeviceToDevice, S(stream)));
  return 0;
}

}  // extern "C"
