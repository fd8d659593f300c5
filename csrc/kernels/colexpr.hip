// colexpr.hip — computed columns of a columnar scan (PG-Strom evaluates
// scalar expressions on the device ahead of its scan, join, pre-aggregate and
// sort stages): one arithmetic expression over up to four source columns,
// evaluated for all record batches of a group in one launch into an 8-byte
// column that every later stage reads like a stored one.  The program, the
// two domains and the output tables are specified in strom.h.
//
// Walk: that of qual_kernel (colfilter.hip) — one wave per 64-row bitmap
// word, one lane per row, kU words per trip with every source load issued
// before the first op.  The result's validity word is the AND of the sources'
// words (one 64-bit load each per wave); one lane stores it, and only lanes
// whose bit is set load and store values.
//
// The program is the same for every lane, so the interpreter's branches are
// scalar.  The operand stack stays in registers: the top of the stack is a
// named value, the seven below it an array that is only ever indexed under a
// switch on the (wave-uniform) depth, every index a constant.  A push or a
// binary op moves one value under that switch; the arithmetic itself exists
// once, outside it.
//
// Every piece is a host-device function: the kernel runs them over the lanes,
// strom_column_expr_host over a loop.  No contraction anywhere in this file:
// a * b + c is two roundings on both sides.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "strom/strom.h"

#pragma clang fp contract(off)

#define HD __host__ __device__ inline

namespace {

constexpr uint32_t kU = 4;             // words of a wave per trip
constexpr uint32_t kBelow = STROM_EXPR_MAX_DEPTH - 1;
constexpr uint64_t kNaN = 0x7ff8000000000000ull;

HD double as_f(uint64_t x) {
  double d;
  __builtin_memcpy(&d, &x, 8);
  return d;
}

HD uint64_t as_u(double d) {
  uint64_t x;
  __builtin_memcpy(&x, &d, 8);
  return x;
}

HD bool int_type(uint32_t t) {
  return t == STROM_COL_I8 || t == STROM_COL_I16 || t == STROM_COL_I32 || t == STROM_COL_I64 ||
         t == STROM_COL_U8 || t == STROM_COL_U16 || t == STROM_COL_U32;
}

// row i of a source column, widened to the domain's 64 bits
template <bool FLT>
HD uint64_t load_src(uint32_t type, uint64_t base, uint64_t i) {
  int64_t v = 0;
  switch (type) {
    case STROM_COL_I8: v = ((const int8_t *)base)[i]; break;
    case STROM_COL_I16: v = ((const int16_t *)base)[i]; break;
    case STROM_COL_I32: v = ((const int32_t *)base)[i]; break;
    case STROM_COL_I64: v = ((const int64_t *)base)[i]; break;
    case STROM_COL_U8: v = ((const uint8_t *)base)[i]; break;
    case STROM_COL_U16: v = ((const uint16_t *)base)[i]; break;
    case STROM_COL_U32: v = ((const uint32_t *)base)[i]; break;
    case STROM_COL_F32:
      if constexpr (FLT) return as_u((double)((const float *)base)[i]);
      break;
    case STROM_COL_F64:
      if constexpr (FLT) return ((const uint64_t *)base)[i];
      break;
    default: break;
  }
  if constexpr (FLT) return as_u((double)v);
  return (uint64_t)v;
}

HD uint64_t int_neg(uint64_t a) { return 0 - a; }
HD uint64_t int_abs(uint64_t a) { return (int64_t)a < 0 ? 0 - a : a; }
// c > 0 (strom_expr_check): the quotient never overflows
HD uint64_t int_fdiv(uint64_t a, uint64_t c) {
  const int64_t x = (int64_t)a, d = (int64_t)c;
  const int64_t q = x / d;
  return (uint64_t)(q - ((x % d) < 0 ? 1 : 0));
}
HD uint64_t int_mod(uint64_t a, uint64_t c) {
  const int64_t x = (int64_t)a, d = (int64_t)c;
  const int64_t r = x % d;
  return (uint64_t)(r < 0 ? r + d : r);
}

template <bool FLT>
HD uint64_t unop(uint32_t op, uint64_t a, uint64_t imm) {
  if constexpr (FLT) {
    return op == STROM_XOP_NEG ? a ^ (1ull << 63) : a & ~(1ull << 63);
  } else {
    switch (op) {
      case STROM_XOP_NEG: return int_neg(a);
      case STROM_XOP_ABS: return int_abs(a);
      case STROM_XOP_FDIV: return int_fdiv(a, imm);
      default: return int_mod(a, imm);
    }
  }
}

template <bool FLT>
HD uint64_t binop(uint32_t op, uint64_t a, uint64_t b) {
  if constexpr (FLT) {
    const double x = as_f(a), y = as_f(b);
    switch (op) {
      case STROM_XOP_ADD: return as_u(x + y);
      case STROM_XOP_SUB: return as_u(x - y);
      case STROM_XOP_MUL: return as_u(x * y);
      default: return as_u(x / y);
    }
  } else {
    switch (op) {
      case STROM_XOP_ADD: return a + b;
      case STROM_XOP_SUB: return a - b;
      default: return a * b;
    }
  }
}

// what is stored: the stack's one value, every NaN as the same bits
template <bool FLT>
HD uint64_t result_of(uint64_t t) {
  if constexpr (FLT) {
    const double d = as_f(t);
    return d != d ? kNaN : t;
  }
  return t;
}

HD bool is_push(uint32_t op) { return op == STROM_XOP_COL || op == STROM_XOP_CONST; }
HD bool is_unary(uint32_t op) {
  return op == STROM_XOP_NEG || op == STROM_XOP_ABS || op == STROM_XOP_FDIV ||
         op == STROM_XOP_MOD;
}
HD bool is_binary(uint32_t op) {
  return op == STROM_XOP_ADD || op == STROM_XOP_SUB || op == STROM_XOP_MUL ||
         op == STROM_XOP_DIV;
}

HD int expr_check(const strom_expr *e) {
  if (!e || e->domain > STROM_EXPR_FLT) return -22;
  if (e->nops < 1 || e->nops > STROM_EXPR_MAX_OPS || e->ncols > STROM_EXPR_MAX_COLS) return -22;
  const bool flt = e->domain == STROM_EXPR_FLT;
  for (uint32_t c = 0; c < e->ncols; ++c) {
    const uint32_t t = e->col_type[c];
    if (!(int_type(t) || (flt && (t == STROM_COL_F32 || t == STROM_COL_F64)))) return -22;
  }
  uint32_t depth = 0;
  for (uint32_t p = 0; p < e->nops; ++p) {
    const strom_expr_op &o = e->ops[p];
    if (is_push(o.op)) {
      if (o.op == STROM_XOP_COL && o.arg >= e->ncols) return -22;
      if (++depth > STROM_EXPR_MAX_DEPTH) return -22;
    } else if (is_unary(o.op)) {
      if (depth < 1) return -22;
      if (o.op == STROM_XOP_FDIV || o.op == STROM_XOP_MOD)
        if (flt || (int64_t)o.imm <= 0) return -22;
    } else if (is_binary(o.op)) {
      if (depth < 2) return -22;
      if (o.op == STROM_XOP_DIV && !flt) return -22;
      --depth;
    } else {
      return -22;
    }
  }
  return depth == 1 ? 0 : -22;
}

// batch of word w: the last b with word_base <= w (uniform per wave)
HD uint32_t batch_of(const strom_filter_batch *b, uint32_t nb, uint64_t w) {
  uint32_t lo = 0, hi = nb;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (b[mid].word_base <= w) lo = mid;
    else hi = mid;
  }
  return lo;
}

// validity of word k of batch bi: the sources' words ANDed, cut to nrows
// (k * 64 < nrows)
HD uint64_t valid_word(const strom_expr &e, const strom_filter_batch *src, uint32_t nb,
                       uint32_t bi, uint64_t nrows, uint64_t k) {
  const uint64_t left = nrows - k * 64;
  uint64_t v = left >= 64 ? ~0ull : (1ull << left) - 1;
  for (uint32_t c = 0; c < e.ncols; ++c) {
    const uint64_t p = src[(uint64_t)c * nb + bi].valid;
    if (p) v &= ((const uint64_t *)p)[k];
  }
  return v;
}

template <bool FLT>
__global__ __launch_bounds__(256) void expr_kernel(strom_expr e,
                                                   const strom_filter_batch *__restrict__ src,
                                                   uint32_t nb, uint64_t nwords,
                                                   const uint64_t *__restrict__ sel,
                                                   const strom_filter_batch *__restrict__ out) {
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint64_t step = (uint64_t)gridDim.x * 4 * kU;
  for (uint64_t w0 = ((uint64_t)blockIdx.x * 4 + wid) * kU; w0 < nwords; w0 += step) {
    // pass 1: batch lookup, the validity word (stored by one lane) and every
    // source value of kU words, all loads issued before the first op
    uint64_t x[STROM_EXPR_MAX_COLS][kU];
    uint64_t dst[kU];
    bool on[kU];
    uint64_t any = 0;
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u) {
      const uint64_t w = w0 + u;
      on[u] = false;
      dst[u] = 0;
#pragma unroll
      for (uint32_t c = 0; c < STROM_EXPR_MAX_COLS; ++c) x[c][u] = 0;
      if (w >= nwords) continue;
      const uint32_t bi = batch_of(out, nb, w);
      const strom_filter_batch &ob = out[bi];
      const uint64_t k = w - ob.word_base;
      if (k * 64 >= ob.nrows) continue;
      uint64_t vword = 0;
      if (!sel || sel[w]) vword = valid_word(e, src, nb, bi, ob.nrows, k);
      if (lane == 0) ((uint64_t *)ob.valid)[k] = vword;
      any |= vword;
      if (!((vword >> lane) & 1)) continue;
      on[u] = true;
      const uint64_t i = k * 64 + lane;
      dst[u] = ob.values + i * 8;
#pragma unroll
      for (uint32_t c = 0; c < STROM_EXPR_MAX_COLS; ++c)
        if (c < e.ncols) x[c][u] = load_src<FLT>(e.col_type[c], src[(uint64_t)c * nb + bi].values, i);
    }
    if (!any) continue;   // uniform: every word null, skipped or past the end
    // pass 2: the program, once for the kU rows of a lane
    uint64_t t[kU], a[kU], s[kBelow][kU];
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u) {
      t[u] = 0;
      a[u] = 0;
#pragma unroll
      for (uint32_t d = 0; d < kBelow; ++d) s[d][u] = 0;
    }
    uint32_t depth = 0;
    for (uint32_t p = 0; p < e.nops; ++p) {
      const uint32_t op = e.ops[p].op, arg = e.ops[p].arg;
      const uint64_t imm = e.ops[p].imm;
      if (is_push(op)) {
#define SPILL(D) case D + 1: _Pragma("unroll") for (uint32_t u = 0; u < kU; ++u) s[D][u] = t[u]; break;
        switch (depth) {
          SPILL(0) SPILL(1) SPILL(2) SPILL(3) SPILL(4) SPILL(5) SPILL(6)
          default: break;
        }
#undef SPILL
        ++depth;
        if (op == STROM_XOP_CONST) {
#pragma unroll
          for (uint32_t u = 0; u < kU; ++u) t[u] = imm;
        } else {
#define COL(C) case C: _Pragma("unroll") for (uint32_t u = 0; u < kU; ++u) t[u] = x[C][u]; break;
          switch (arg) {
            COL(0) COL(1) COL(2)
            default: COL(3)
          }
#undef COL
        }
      } else if (is_unary(op)) {
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u) t[u] = unop<FLT>(op, t[u], imm);
      } else {
#define FETCH(D) case D + 2: _Pragma("unroll") for (uint32_t u = 0; u < kU; ++u) a[u] = s[D][u]; break;
        switch (depth) {
          FETCH(0) FETCH(1) FETCH(2) FETCH(3) FETCH(4) FETCH(5) FETCH(6)
          default: break;
        }
#undef FETCH
        --depth;
#pragma unroll
        for (uint32_t u = 0; u < kU; ++u) t[u] = binop<FLT>(op, a[u], t[u]);
      }
    }
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u)
      if (on[u]) *(uint64_t *)dst[u] = result_of<FLT>(t[u]);
  }
}

template <bool FLT>
void host_walk(const strom_expr &e, const strom_filter_batch *src, uint32_t nb, uint64_t nwords,
               const uint64_t *sel, const strom_filter_batch *out) {
  for (uint64_t w = 0; w < nwords; ++w) {
    const uint32_t bi = batch_of(out, nb, w);
    const strom_filter_batch &ob = out[bi];
    const uint64_t k = w - ob.word_base;
    if (k * 64 >= ob.nrows) continue;
    uint64_t vword = 0;
    if (!sel || sel[w]) vword = valid_word(e, src, nb, bi, ob.nrows, k);
    ((uint64_t *)ob.valid)[k] = vword;
    for (uint32_t lane = 0; lane < 64; ++lane) {
      if (!((vword >> lane) & 1)) continue;
      const uint64_t i = k * 64 + lane;
      uint64_t s[STROM_EXPR_MAX_DEPTH];
      uint32_t depth = 0;
      for (uint32_t p = 0; p < e.nops; ++p) {
        const strom_expr_op &o = e.ops[p];
        if (o.op == STROM_XOP_CONST) {
          s[depth++] = o.imm;
        } else if (o.op == STROM_XOP_COL) {
          s[depth++] = load_src<FLT>(e.col_type[o.arg], src[(uint64_t)o.arg * nb + bi].values, i);
        } else if (is_unary(o.op)) {
          s[depth - 1] = unop<FLT>(o.op, s[depth - 1], o.imm);
        } else {
          s[depth - 2] = binop<FLT>(o.op, s[depth - 2], s[depth - 1]);
          --depth;
        }
      }
      ((uint64_t *)ob.values)[i] = result_of<FLT>(s[0]);
    }
  }
}

bool args_ok(const strom_expr *e, const strom_filter_batch *src, uint32_t nb,
             const uint64_t *sel, const strom_filter_batch *out) {
  if (expr_check(e) != 0) return false;
  if (!out || !nb || (e->ncols && !src)) return false;
  return !(((uintptr_t)src | (uintptr_t)out | (uintptr_t)sel) & 7);
}

}  // namespace

extern "C" int strom_expr_check(const strom_expr *e) { return expr_check(e); }

extern "C" int strom_column_expr(const strom_expr *e, const strom_filter_batch *d_src,
                                 uint32_t nbatches, uint64_t nwords, const uint64_t *d_sel,
                                 const strom_filter_batch *d_out, void *stream) {
  if (!args_ok(e, d_src, nbatches, d_sel, d_out)) return -22;
  if (!nwords) return 0;
  const uint64_t g = (nwords + 4 * kU - 1) / (4 * kU);
  const uint32_t grid = (uint32_t)(g > 8192 ? 8192 : g);
  hipStream_t st = (hipStream_t)stream;
  if (e->domain == STROM_EXPR_FLT)
    hipLaunchKernelGGL(expr_kernel<true>, dim3(grid), dim3(256), 0, st, *e, d_src, nbatches, nwords,
                       d_sel, d_out);
  else
    hipLaunchKernelGGL(expr_kernel<false>, dim3(grid), dim3(256), 0, st, *e, d_src, nbatches,
                       nwords, d_sel, d_out);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int strom_column_expr_host(const strom_expr *e, const strom_filter_batch *src,
                                      uint32_t nbatches, uint64_t nwords, const uint64_t *sel,
                                      const strom_filter_batch *out) {
  if (!args_ok(e, src, nbatches, sel, out)) return -22;
  if (e->domain == STROM_EXPR_FLT) host_walk<true>(*e, src, nbatches, nwords, sel, out);
  else host_walk<false>(*e, src, nbatches, nwords, sel, out);
  return 0;
}
