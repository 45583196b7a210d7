// ETL: the OTTO jsonl session and label files -> integer columns in HBM (etl/jsonl_to_parquet.py:23-56).
//
// A piece of the file (whole lines, n_bytes < 2^31, 16-byte aligned) is parsed in count, scan, write order:
//   k_jsonl_marks<.., false> : every lane loads 16 B; a wave classifies its 1024-byte tile into line ends ('\n') and
//                              marks (sessions: a '{' that does not open its line = an event; labels: the first
//                              digit of a number) and stores one packed (lines << 32 | marks) count per tile
//   exclusive_scan_u64       : over the n_bytes / 1024 tile counts (no per-byte flag or index arrays)
//   k_jsonl_marks<.., true>  : the same tiling; every line start and mark goes to (tile base + rank in the tile):
//                              line_pos, line_ev (marks before the line), ev_pos, ev_line
//   sessions: k_jsonl_events : one lane per event walks its object through '}' and the separator after it
//             k_jsonl_lines  : one lane per line walks the header and, from where the last event stopped, the tail
//             k_jsonl_fill   : session[e] = the id its line lane parsed
//   labels:   k_labels_cap, scan, k_labels_lines : one lane per line, rows at the scanned row base of the line
// Row and line order come from the scans alone, so the output is the same bytes on every run; the only atomic is
// the atomicMin that keeps the first bad byte. A block of event lanes first stages the text of its 256 events in
// LDS with 16-byte loads and walks that copy (measured against byte loads from global memory: DESIGN.md, ETL); the
// line lanes, whose bytes are few and far apart, read global memory.
// Every byte of the piece is walked by exactly one lane that expects a definite set of bytes there, so a byte
// outside the strict grammar of DESIGN.md is an error wherever it stands.
// The tile passes (k_jsonl_marks, jsonl_count, jsonl_locate) are in text_marks.h, shared with submit.hip.
#include <algorithm>
#include "prims.h"
#include "table.h"
#include "text_marks.h"

namespace ottohip {

enum : uint32_t {
  JE_BYTE = 1,  // a byte the grammar does not allow here
  JE_KEY,       // unknown key
  JE_DUP,       // key given twice
  JE_MISSING,   // key missing
  JE_ZERO,      // leading zero
  JE_TYPE,      // type not clicks / carts / orders
  JE_CUT,       // the text ends inside a line
  JE_STRUCT,    // brackets do not close where the line's values end
  JE_DIGITS,    // from here: OTTOHIP_ELIMIT. more than 18 digits
  JE_AID,       // aid above int32
  JE_TS,        // ts / 1000 above int32
  JE_SESSION,   // session above int32
};
static const char* const JE_TEXT[] = {"", "unexpected byte", "unknown key", "duplicate key", "missing key",
                                      "leading zero", "type is not clicks, carts or orders", "text ends inside the line",
                                      "brackets do not match the line's values", "number of more than 18 digits",
                                      "aid does not fit int32", "ts in seconds does not fit int32",
                                      "session does not fit int32"};
constexpr unsigned long long JE_NONE = ~0ull;

__device__ __forceinline__ void je_fail(unsigned long long* err, uint32_t off, uint32_t why) {
  atomicMin(err, ((unsigned long long)off << 8) | why);
}

// A lane's read position in the piece. Every read is below n; p never passes n. Bytes of [w0, w0 + wlen) come
// from the block's staged copy in LDS when there is one.
struct Cur {
  const uint8_t* __restrict__ t;
  uint32_t p, n;
  unsigned long long* err;
  const uint8_t* lds = nullptr;
  uint32_t w0 = 0, wlen = 0;
  __device__ __forceinline__ int at(uint32_t q) const { return q - w0 < wlen ? (int)lds[q - w0] : (int)t[q]; }
  __device__ __forceinline__ int peek() const { return p < n ? at(p) : -1; }
  __device__ __forceinline__ int peek1() const { return p + 1u < n ? at(p + 1u) : -1; }
  __device__ __forceinline__ void ws() {
    while (p < n && is_ws(at(p))) ++p;
  }
  __device__ __forceinline__ bool bad(uint32_t why) {
    je_fail(err, p, p >= n ? (uint32_t)JE_CUT : why);
    return false;
  }
  __device__ __forceinline__ bool expect(int c) {
    if (peek() == c) { ++p; return true; }
    return bad(JE_BYTE);
  }
  __device__ __forceinline__ bool lit(const char* s, int len, uint32_t why) {
    for (int i = 0; i < len; ++i) {
      if (peek() != (int)s[i]) return bad(why);
      ++p;
    }
    return true;
  }
  // 0 | [1-9][0-9]{0,17}
  __device__ __forceinline__ bool integer(int64_t* v) {
    int c = peek();
    if (!is_digit(c)) return bad(JE_BYTE);
    if (c == '0') {
      ++p;
      if (is_digit(peek())) return bad(JE_ZERO);
      *v = 0;
      return true;
    }
    int64_t x = 0;
    for (int d = 0; is_digit(c = peek()); ++d) {
      if (d == 18) return bad(JE_DIGITS);
      x = x * 10 + (c - '0');
      ++p;
    }
    *v = x;
    return true;
  }
  // "clicks" | "carts" | "orders", from the opening quote through the closing one
  __device__ __forceinline__ bool type_name(int* ty) {
    if (!expect('"')) return false;
    const int c = peek();
    if (c == 'c') {
      if (peek1() == 'l') { *ty = 0; return lit("clicks\"", 7, JE_TYPE); }
      *ty = 1;
      return lit("carts\"", 6, JE_TYPE);
    }
    *ty = 2;
    return lit("orders\"", 7, JE_TYPE);
  }
};

// one lane per event: '{' at ev_pos[e] through '}' and what follows it (", {" or "]"). The block first copies the
// text of its 256 events (from the first one's '{' to the '{' behind the last one's, at most JSONL_STAGE bytes; 256
// events of the data set's style are 13 KB) into LDS with 16-byte loads; the lanes then walk that copy, and the
// global text only past its end
constexpr uint32_t JSONL_STAGE = 32768;
__global__ __launch_bounds__(JSONL_T) void k_jsonl_events(const uint8_t* __restrict__ text, uint32_t n,
                                                          const uint32_t* __restrict__ ev_pos,
                                                          const uint32_t* __restrict__ ev_line, int64_t n_ev,
                                                          int32_t* __restrict__ aid, int32_t* __restrict__ ts,
                                                          int8_t* __restrict__ type, uint32_t* __restrict__ ev_end,
                                                          unsigned long long* __restrict__ err) {
  __shared__ uint4 stage[JSONL_STAGE / 16];
  const int64_t first = (int64_t)blockIdx.x * JSONL_T, e = first + threadIdx.x;
  const int64_t stop = first + JSONL_T;
  const uint32_t w0 = ev_pos[first] & ~15u;  // the piece is 16-byte aligned, so these loads are too
  const uint32_t wend = stop < n_ev ? ev_pos[stop] + 1u : n;
  const uint32_t wlen = min((wend - w0 + 15u) & ~15u, JSONL_STAGE);
  for (uint32_t i = threadIdx.x; i * 16u < wlen; i += JSONL_T) {
    const uint32_t o = w0 + i * 16u;  // below wend, so below n
    uint4 v = make_uint4(0, 0, 0, 0);
    if (o + 16u <= n) {
      v = *reinterpret_cast<const uint4*>(text + o);
    } else {  // the piece's last, short chunk: nothing read at or after n
      uint32_t w[4] = {0, 0, 0, 0};
      for (uint32_t j = 0; o + j < n; ++j) w[j >> 2] |= (uint32_t)text[o + j] << ((j & 3) * 8);
      v = make_uint4(w[0], w[1], w[2], w[3]);
    }
    stage[i] = v;
  }
  __syncthreads();
  if (e >= n_ev) return;
  Cur c{text, ev_pos[e] + 1u, n, err, reinterpret_cast<const uint8_t*>(stage), w0, wlen};
  int64_t va = 0, vt = 0;
  int ty = 0;
  uint32_t seen = 0;
  for (;;) {
    c.ws();
    const uint32_t at = c.p;
    if (!c.expect('"')) return;
    int k;
    const int ch = c.peek();
    if (ch == 'a') {
      if (!c.lit("aid\"", 4, JE_KEY)) return;
      k = 0;
    } else if (ch == 't' && c.peek1() == 's') {
      if (!c.lit("ts\"", 3, JE_KEY)) return;
      k = 1;
    } else {
      if (!c.lit("type\"", 5, JE_KEY)) return;
      k = 2;
    }
    if (seen & (1u << k)) { je_fail(err, at, JE_DUP); return; }
    seen |= 1u << k;
    c.ws();
    if (!c.expect(':')) return;
    c.ws();
    const uint32_t vat = c.p;
    if (k == 0) {
      if (!c.integer(&va)) return;
      if (va > 2147483647ll) { je_fail(err, vat, JE_AID); return; }
    } else if (k == 1) {
      if (!c.integer(&vt)) return;
      if (vt / 1000 > 2147483647ll) { je_fail(err, vat, JE_TS); return; }
    } else {
      if (!c.type_name(&ty)) return;
    }
    c.ws();
    const int sep = c.peek();
    if (sep == ',') { ++c.p; continue; }
    if (sep == '}') break;
    c.bad(JE_BYTE);
    return;
  }
  if (seen != 7u) { je_fail(err, c.p, JE_MISSING); return; }
  ++c.p;  // '}'
  c.ws();
  const int nx = c.peek();
  if (nx == ',') {
    ++c.p;
    c.ws();
    if (c.peek() != '{') { c.bad(JE_BYTE); return; }  // the next event's lane takes it from there
  } else if (nx == ']') {
    if (e + 1 < n_ev && ev_line[e + 1] == ev_line[e]) { je_fail(err, c.p, JE_STRUCT); return; }  // not the line's last
    ++c.p;
    ev_end[e] = c.p;
  } else {
    c.bad(JE_BYTE);
    return;
  }
  aid[e] = (int32_t)va;
  ts[e] = (int32_t)(vt / 1000);
  type[e] = (int8_t)ty;
}

// one lane per line: the header through '[', and the tail from behind the ']' its last event stopped at.
// rows[l] = events of the line, or -1 for a blank line
__global__ __launch_bounds__(JSONL_T) void k_jsonl_lines(const uint8_t* __restrict__ text, uint32_t n,
                                                         const uint32_t* __restrict__ line_pos,
                                                         const uint32_t* __restrict__ line_ev, int64_t n_lines,
                                                         const uint32_t* __restrict__ ev_pos,
                                                         const uint32_t* __restrict__ ev_end,
                                                         int32_t* __restrict__ line_session, int64_t* __restrict__ rows,
                                                         unsigned long long* __restrict__ err) {
  const int64_t l = (int64_t)blockIdx.x * JSONL_T + threadIdx.x;
  if (l >= n_lines) return;
  Cur c{text, line_pos[l], n, err};
  const uint32_t e0 = line_ev[l], e1 = line_ev[l + 1];
  c.ws();
  if (c.peek() == '\n' || c.peek() < 0) {  // blank; it holds no '{', so no event lane runs in it
    if (rows) rows[l] = -1;
    return;
  }
  if (!c.expect('{')) return;
  int64_t sid = 0;
  uint32_t seen = 0;
  for (;;) {
    c.ws();
    const uint32_t at = c.p;
    if (!c.expect('"')) return;
    int k;
    if (c.peek() == 's') {
      if (!c.lit("session\"", 8, JE_KEY)) return;
      k = 0;
    } else {
      if (!c.lit("events\"", 7, JE_KEY)) return;
      k = 1;
    }
    if (seen & (1u << k)) { je_fail(err, at, JE_DUP); return; }
    seen |= 1u << k;
    c.ws();
    if (!c.expect(':')) return;
    c.ws();
    if (k == 0) {
      const uint32_t vat = c.p;
      if (!c.integer(&sid)) return;
      if (sid > 2147483647ll) { je_fail(err, vat, JE_SESSION); return; }
    } else {
      if (!c.expect('[')) return;
      c.ws();
      const int ch = c.peek();
      if (ch == ']') {
        ++c.p;
      } else if (ch == '{') {
        // this brace is the line's first event; its lanes walked on to the ']' behind the last one
        if (e0 >= e1 || ev_pos[e0] != c.p) { c.bad(JE_STRUCT); return; }
        const uint32_t end = ev_end[e1 - 1u];
        if (end == 0u) {  // an event lane of this line stopped at its own error; this one ranks behind it
          je_fail(err, line_pos[l + 1] > 0u ? line_pos[l + 1] - 1u : 0u, JE_STRUCT);
          return;
        }
        c.p = end;
      } else {
        c.bad(JE_BYTE);
        return;
      }
    }
    c.ws();
    const int sep = c.peek();
    if (sep == ',') { ++c.p; continue; }
    if (sep == '}') break;
    c.bad(JE_BYTE);
    return;
  }
  if (seen != 3u) { je_fail(err, c.p, JE_MISSING); return; }
  ++c.p;  // '}'
  c.ws();
  if (c.peek() != '\n' && c.peek() >= 0) { c.bad(JE_BYTE); return; }
  line_session[l] = (int32_t)sid;
  if (rows) rows[l] = (int64_t)(e1 - e0);
}

__global__ void k_jsonl_fill(const uint32_t* __restrict__ ev_line, int64_t n_ev,
                             const int32_t* __restrict__ line_session, int32_t* __restrict__ session) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n_ev) session[e] = line_session[ev_line[e]];
}

// labels: a line holds one number for the session and one per row
__global__ void k_labels_cap(const uint32_t* __restrict__ line_ev, int64_t n_lines, uint32_t* __restrict__ cap) {
  const int64_t l = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= n_lines) return;
  const uint32_t d = line_ev[l + 1] - line_ev[l];
  cap[l] = d > 0u ? d - 1u : 0u;
}

// one lane per labels line; rows [row0[l], row0[l] + cap[l]) are the line's
__global__ __launch_bounds__(JSONL_T) void k_labels_lines(const uint8_t* __restrict__ text, uint32_t n,
                                                          const uint32_t* __restrict__ line_pos, int64_t n_lines,
                                                          const uint32_t* __restrict__ cap,
                                                          const uint64_t* __restrict__ row0,
                                                          int32_t* __restrict__ session, int8_t* __restrict__ type,
                                                          int32_t* __restrict__ aid, int64_t* __restrict__ rows,
                                                          unsigned long long* __restrict__ err) {
  const int64_t l = (int64_t)blockIdx.x * JSONL_T + threadIdx.x;
  if (l >= n_lines) return;
  Cur c{text, line_pos[l], n, err};
  c.ws();
  if (c.peek() == '\n' || c.peek() < 0) {
    if (rows) rows[l] = -1;
    return;
  }
  const uint64_t r0 = row0[l];
  const uint32_t room = cap[l];
  uint32_t used = 0;
  if (!c.expect('{')) return;
  int64_t sid = 0;
  uint32_t seen = 0;
  for (;;) {
    c.ws();
    const uint32_t at = c.p;
    if (!c.expect('"')) return;
    int k;
    if (c.peek() == 's') {
      if (!c.lit("session\"", 8, JE_KEY)) return;
      k = 0;
    } else {
      if (!c.lit("labels\"", 7, JE_KEY)) return;
      k = 1;
    }
    if (seen & (1u << k)) { je_fail(err, at, JE_DUP); return; }
    seen |= 1u << k;
    c.ws();
    if (!c.expect(':')) return;
    c.ws();
    if (k == 0) {
      const uint32_t vat = c.p;
      if (!c.integer(&sid)) return;
      if (sid > 2147483647ll) { je_fail(err, vat, JE_SESSION); return; }
    } else {
      if (!c.expect('{')) return;
      c.ws();
      uint32_t types = 0;
      if (c.peek() == '}') {
        ++c.p;
      } else {
        for (;;) {  // "type" : int | [ int, ... ]
          c.ws();
          const uint32_t tat = c.p;
          int ty;
          if (!c.type_name(&ty)) return;
          if (types & (1u << ty)) { je_fail(err, tat, JE_DUP); return; }
          types |= 1u << ty;
          c.ws();
          if (!c.expect(':')) return;
          c.ws();
          const bool list = c.peek() == '[';
          if (list) {
            ++c.p;
            c.ws();
          }
          if (list && c.peek() == ']') {
            ++c.p;
          } else {
            for (;;) {
              const uint32_t vat = c.p;
              int64_t v;
              if (!c.integer(&v)) return;
              if (v > 2147483647ll) { je_fail(err, vat, JE_AID); return; }
              if (used >= room) { je_fail(err, vat, JE_STRUCT); return; }  // more numbers than the count pass saw
              aid[r0 + used] = (int32_t)v;
              type[r0 + used] = (int8_t)ty;
              ++used;
              if (!list) break;
              c.ws();
              const int sep = c.peek();
              if (sep == ',') { ++c.p; c.ws(); continue; }
              if (sep == ']') { ++c.p; break; }
              c.bad(JE_BYTE);
              return;
            }
          }
          c.ws();
          const int sep = c.peek();
          if (sep == ',') { ++c.p; continue; }
          if (sep == '}') { ++c.p; break; }
          c.bad(JE_BYTE);
          return;
        }
      }
    }
    c.ws();
    const int sep = c.peek();
    if (sep == ',') { ++c.p; continue; }
    if (sep == '}') break;
    c.bad(JE_BYTE);
    return;
  }
  if (seen != 3u) { je_fail(err, c.p, JE_MISSING); return; }
  ++c.p;  // '}'
  c.ws();
  if (c.peek() != '\n' && c.peek() >= 0) { c.bad(JE_BYTE); return; }
  if (used != room) { je_fail(err, line_pos[l], JE_STRUCT); return; }
  for (uint32_t i = 0; i < used; ++i) session[r0 + i] = (int32_t)sid;
  if (rows) rows[l] = (int64_t)used;
}

// ---------------------------------------------------------------- host side
// reads the first-error word; on an error names the line (line_base + its index in the piece + 1) and the byte
static int jsonl_verdict(const char* who, const unsigned long long* err, const JsonlScan& J, int64_t line_base,
                         hipStream_t s) {
  unsigned long long h = 0;
  OH_TRY(d2h(&h, err, 1, s));
  if (h == JE_NONE) return 0;
  const uint32_t off = (uint32_t)(h >> 8), why = (uint32_t)(h & 0xFFu);
  std::vector<uint32_t> lp((size_t)J.n_lines);
  OH_TRY(d2h(lp.data(), J.line_pos, (size_t)J.n_lines, s));
  const int64_t li = (int64_t)(std::upper_bound(lp.begin(), lp.end(), off) - lp.begin()) - 1;
  set_error("%s: line %lld, byte %lld of the piece: %s", who, (long long)(line_base + li + 1), (long long)off,
            why < sizeof JE_TEXT / sizeof JE_TEXT[0] ? JE_TEXT[why] : "?");
  return why >= JE_DIGITS ? OTTOHIP_ELIMIT : OTTOHIP_EINVAL;
}

static int labels_rows(Ctx* ctx, JsonlScan& J, uint32_t** cap, uint64_t** row0, int64_t* n_rows, hipStream_t s) {
  uint64_t* tot;
  OH_TRY(ctx->ws.get("jl_cap", (size_t)J.n_lines, cap));
  OH_TRY(ctx->ws.get("jl_row0", (size_t)J.n_lines, row0));
  OH_TRY(ctx->ws.get("jl_rtot", 1, &tot));
  k_labels_cap<<<grid_for(J.n_lines), 256, 0, s>>>(J.line_ev, J.n_lines, *cap);
  OH_HIP(hipGetLastError());
  OH_TRY(exclusive_scan_u32(ctx, *cap, *row0, J.n_lines, tot, s));
  uint64_t t = 0;
  OH_TRY(d2h(&t, tot, 1, s));
  *n_rows = (int64_t)t;
  return 0;
}

}  // namespace ottohip

using namespace ottohip;

extern "C" int ottohip_jsonl_tile_bytes(void) { return JSONL_TILE_BYTES; }

extern "C" int ottohip_jsonl_count(ottohip_ctx* c, const uint8_t* text, int64_t n_bytes, int kind, int64_t* n_lines,
                                   int64_t* n_rows, void* stream) {
  OH_TRY(jsonl_args("jsonl_count", c, text, n_bytes));
  if (!n_lines || !n_rows || (kind != 0 && kind != 1)) { set_error("jsonl_count: bad arguments"); return OTTOHIP_EINVAL; }
  *n_lines = *n_rows = 0;
  if (n_bytes == 0) return 0;
  hipStream_t s = S(stream);
  OH_HIP(hipSetDevice(c->device));
  c->reset_timing();
  JsonlScan J;
  if (kind == 0) {
    OH_TRY(jsonl_count<0>(c, text, n_bytes, J, s));
    *n_rows = J.n_marks;
  } else {
    uint32_t* cap;
    uint64_t* row0;
    OH_TRY(jsonl_count<1>(c, text, n_bytes, J, s));
    OH_TRY(jsonl_locate<1>(c, text, n_bytes, J, s));
    OH_TRY(labels_rows(c, J, &cap, &row0, n_rows, s));
  }
  *n_lines = J.n_lines;
  return 0;
}

extern "C" int ottohip_jsonl_sessions(ottohip_ctx* c, const uint8_t* text, int64_t n_bytes, int64_t line_base,
                                      int32_t* session, int32_t* aid, int32_t* ts, int8_t* type,
                                      int64_t* rows_per_line, int64_t cap_rows, int64_t cap_lines, void* stream) {
  OH_TRY(jsonl_args("jsonl_sessions", c, text, n_bytes));
  if (line_base < 0 || cap_rows < 0 || cap_lines < 0 || (cap_rows > 0 && (!session || !aid || !ts || !type))) {
    set_error("jsonl_sessions: bad arguments");
    return OTTOHIP_EINVAL;
  }
  if (n_bytes == 0) return 0;
  hipStream_t s = S(stream);
  OH_HIP(hipSetDevice(c->device));
  c->reset_timing();
  Workspace& ws = c->ws;
  JsonlScan J;
  OH_TRY(jsonl_count<0>(c, text, n_bytes, J, s));
  if (J.n_marks > cap_rows || (rows_per_line && J.n_lines > cap_lines)) {
    set_error("jsonl_sessions: %lld rows in %lld lines, buffers of %lld and %lld", (long long)J.n_marks,
              (long long)J.n_lines, (long long)cap_rows, (long long)cap_lines);
    return OTTOHIP_EINVAL;
  }
  OH_TRY(jsonl_locate<0>(c, text, n_bytes, J, s));
  unsigned long long* err;
  uint32_t* ev_end;
  int32_t* line_session;
  OH_TRY(ws.get("jl_err", 1, &err));
  OH_TRY(ws.get("jl_ev_end", (size_t)std::max<int64_t>(J.n_marks, 1), &ev_end));
  OH_TRY(ws.get("jl_line_session", (size_t)J.n_lines, &line_session));
  OH_HIP(hipMemsetAsync(err, 0xFF, sizeof(unsigned long long), s));
  OH_HIP(hipMemsetAsync(ev_end, 0, (size_t)std::max<int64_t>(J.n_marks, 1) * 4, s));
  OH_HIP(hipMemsetAsync(line_session, 0, (size_t)J.n_lines * 4, s));
  const int ph = c->begin("jsonl_parse", s, (double)n_bytes + 13.0 * (double)J.n_marks + 8.0 * (double)(J.n_marks + J.n_lines));
  if (J.n_marks > 0) {
    k_jsonl_events<<<grid_for(J.n_marks, JSONL_T), JSONL_T, 0, s>>>(text, (uint32_t)n_bytes, J.ev_pos, J.ev_line,
                                                                     J.n_marks, aid, ts, type, ev_end, err);
    OH_HIP(hipGetLastError());
  }
  k_jsonl_lines<<<grid_for(J.n_lines, JSONL_T), JSONL_T, 0, s>>>(text, (uint32_t)n_bytes, J.line_pos, J.line_ev,
                                                                  J.n_lines, J.ev_pos, ev_end, line_session,
                                                                  rows_per_line, err);
  OH_HIP(hipGetLastError());
  if (J.n_marks > 0) {
    k_jsonl_fill<<<grid_for(J.n_marks), 256, 0, s>>>(J.ev_line, J.n_marks, line_session, session);
    OH_HIP(hipGetLastError());
  }
  c->end(ph, s);
  return jsonl_verdict("jsonl_sessions", err, J, line_base, s);
}

extern "C" int ottohip_jsonl_labels(ottohip_ctx* c, const uint8_t* text, int64_t n_bytes, int64_t line_base,
                                    int32_t* session, int8_t* type, int32_t* aid, int64_t* rows_per_line,
                                    int64_t cap_rows, int64_t cap_lines, void* stream) {
  OH_TRY(jsonl_args("jsonl_labels", c, text, n_bytes));
  if (line_base < 0 || cap_rows < 0 || cap_lines < 0 || (cap_rows > 0 && (!session || !aid || !type))) {
    set_error("jsonl_labels: bad arguments");
    return OTTOHIP_EINVAL;
  }
  if (n_bytes == 0) return 0;
  hipStream_t s = S(stream);
  OH_HIP(hipSetDevice(c->device));
  c->reset_timing();
  JsonlScan J;
  uint32_t* cap;
  uint64_t* row0;
  int64_t n_rows = 0;
  OH_TRY(jsonl_count<1>(c, text, n_bytes, J, s));
  OH_TRY(jsonl_locate<1>(c, text, n_bytes, J, s));
  OH_TRY(labels_rows(c, J, &cap, &row0, &n_rows, s));
  if (n_rows > cap_rows || (rows_per_line && J.n_lines > cap_lines)) {
    set_error("jsonl_labels: %lld rows in %lld lines, buffers of %lld and %lld", (long long)n_rows,
              (long long)J.n_lines, (long long)cap_rows, (long long)cap_lines);
    return OTTOHIP_EINVAL;
  }
  unsigned long long* err;
  OH_TRY(c->ws.get("jl_err", 1, &err));
  OH_HIP(hipMemsetAsync(err, 0xFF, sizeof(unsigned long long), s));
  const int ph = c->begin("jsonl_parse", s, (double)n_bytes + 9.0 * (double)n_rows + 20.0 * (double)J.n_lines);
  k_labels_lines<<<grid_for(J.n_lines, JSONL_T), JSONL_T, 0, s>>>(text, (uint32_t)n_bytes, J.line_pos, J.n_lines, cap,
                                                                   row0, session, type, aid, rows_per_line, err);
  OH_HIP(hipGetLastError());
  c->end(ph, s);
  return jsonl_verdict("jsonl_labels", err, J, line_base, s);
}
