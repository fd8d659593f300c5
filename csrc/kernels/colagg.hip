// colagg.hip — COUNT / SUM / MIN / MAX over the selection bitmap of a
// columnar scan, optionally GROUP BY a small key domain (PG-Strom feeds its
// scan into GpuPreAgg; this is that stage for the Arrow path).
//
// The qualifier kernels (colfilter.hip) leave a bitmap, 64 rows per word,
// every record batch on fresh words.  These kernels walk the words the same
// way — one wave per word, kU words per trip with their value loads issued
// before the first use, a word whose bitmap is zero costs no value load (that
// skip is a branch on the loaded word: the walk is latency-bound at 0.40 of
// the filter kernel, profiles/r7/agg/SUMMARY.md) — and leave a few kilobytes
// of accumulators:
//
//   no key    each lane accumulates in registers over the whole walk; the
//             wave is reduced with a fixed xor-shuffle tree, the workgroup
//             through LDS in wave order.
//   with key  workgroup-private accumulators in LDS, updated with LDS
//             atomics (integer add / min / max on order-preserving keys,
//             ds_add_f64 for float sums).  Two measures against every lane
//             hitting the same few LDS words:
//             - R replicas of the accumulator set (R = 256 / 128 / ... / 1,
//               as many as fit 64 KiB), a lane uses replica tid % R: a
//               3-slot key gets a private set per lane;
//             - a word whose selected rows all carry ONE key (skewed or
//               clustered data) is accumulated in registers like the
//               unkeyed walk, and flushed with one wave reduction when the
//               key changes.
//
// Workgroups never meet in global float atomics (their sums would depend
// on arrival order, and one hot row runs 14x below the streaming rate): each
// stores its partial accumulators as a slab, and a small reduce kernel folds
// the slabs into the scan's accumulator block in a fixed order.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "strom/strom.h"

namespace {

constexpr uint32_t kU = 4;          // words per wave and trip (as colfilter.hip)
constexpr uint32_t kMaxGrid = 8192;      // as the filter kernels: the walk is latency-bound below it
constexpr uint64_t kSign = 1ull << 63;

struct NoneT {};                    // STROM_COL_NONE: validity only

__device__ __forceinline__ uint32_t batch_of(const strom_filter_batch *b, uint32_t nb, uint64_t w) {
  uint32_t lo = 0, hi = nb;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (b[mid].word_base <= w) lo = mid;
    else hi = mid;
  }
  return lo;
}

// value traits: the sum's type, the widened value, its order-preserving key
template <typename T> struct Tr {
  static constexpr bool flt = std::is_floating_point<T>::value;
  typedef typename std::conditional<flt, double, uint64_t>::type sum_t;
  __device__ static __forceinline__ sum_t widen(T x) {
    if constexpr (flt) return (double)x;
    else if constexpr (std::is_signed<T>::value) return (uint64_t)(int64_t)x;
    else return (uint64_t)x;
  }
  __device__ static __forceinline__ uint64_t key(sum_t s) {
    if constexpr (flt) {
      const uint64_t b = (uint64_t)__double_as_longlong(s);
      return (b & kSign) ? ~b : (b | kSign);
    } else if constexpr (std::is_signed<T>::value) return s ^ kSign;
    else return s;
  }
  __device__ static __forceinline__ bool nan(sum_t s) {
    if constexpr (flt) return s != s;
    else return false;
  }
};
template <> struct Tr<NoneT> {
  static constexpr bool flt = false;
  typedef uint64_t sum_t;
};

__device__ __forceinline__ uint64_t umin64(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }

template <typename S> __device__ __forceinline__ S wave_sum(S v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ uint64_t wave_min(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = umin64(v, (uint64_t)__shfl_xor((unsigned long long)v, o, 64));
  return v;
}
__device__ __forceinline__ uint64_t wave_max(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = umax64(v, (uint64_t)__shfl_xor((unsigned long long)v, o, 64));
  return v;
}

template <typename S> __device__ __forceinline__ uint64_t sum_bits(S s) {
  if constexpr (std::is_same<S, double>::value) return (uint64_t)__double_as_longlong(s);
  else return s;
}

__device__ __forceinline__ uint32_t nacc_of(uint32_t ops) { return __popc(ops & 15u); }

// rows of batch word k that exist
__device__ __forceinline__ uint64_t row_mask(const strom_filter_batch &b, uint64_t k) {
  if (k * 64 >= b.nrows) return 0;
  const uint64_t rem = b.nrows - k * 64;
  return rem >= 64 ? ~0ull : (1ull << rem) - 1;
}

// what one word contributes: the selected rows that exist (sel) and, of
// those, the ones the aggregated column has a value for (use)
struct WordIn {
  uint64_t sel, use;
  uint32_t bi;
  uint64_t k;
};

__device__ __forceinline__ WordIn word_in(const uint64_t *bm, uint64_t nwords, uint64_t w,
                                          const strom_filter_batch *vt, uint32_t nb, bool all) {
  WordIn r{0, 0, 0, 0};
  if (w >= nwords) return r;
  const uint64_t word = bm[w];                       // uniform load, one per wave
  if (!word) return r;
  r.bi = batch_of(vt, nb, w);
  const strom_filter_batch &b = vt[r.bi];
  r.k = w - b.word_base;
  r.sel = word & row_mask(b, r.k);
  r.use = r.sel;
  if (!all && b.valid && r.sel) r.use &= ((const uint64_t *)b.valid)[r.k];
  return r;
}

// ------------------------------------------------------------------ no key
template <typename T>
__global__ __launch_bounds__(256) void agg_flat_kernel(const uint64_t *__restrict__ bm,
                                                       uint64_t nwords,
                                                       const strom_filter_batch *__restrict__ vt,
                                                       uint32_t nb, uint32_t ops,
                                                       uint64_t *__restrict__ slabs) {
  typedef typename Tr<T>::sum_t S;
  constexpr bool kVals = !std::is_same<T, NoneT>::value;
  __shared__ uint64_t red[4][4];
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const bool all = ops & STROM_AGG_ALL;
  uint64_t cnt = 0;                                  // wave-uniform
  S sum = 0;
  uint64_t mnk = ~0ull, mxk = 0;
  const uint64_t step = (uint64_t)gridDim.x * 4 * kU;
  for (uint64_t w0 = ((uint64_t)blockIdx.x * 4 + wid) * kU; w0 < nwords; w0 += step) {
    WordIn in[kU];
    S x[kU];
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u) {
      in[u] = word_in(bm, nwords, w0 + u, vt, nb, all);
      x[u] = 0;
      if constexpr (kVals)
        if ((in[u].use >> lane) & 1)
          x[u] = Tr<T>::widen(((const T *)vt[in[u].bi].values)[in[u].k * 64 + lane]);
    }
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u) {
      if (!in[u].use) continue;
      cnt += __popcll(in[u].use);
      if constexpr (kVals) {
        if ((in[u].use >> lane) & 1) {
          sum += x[u];
          if (!Tr<T>::nan(x[u])) {
            const uint64_t k = Tr<T>::key(x[u]);
            mnk = umin64(mnk, k);
            mxk = umax64(mxk, k);
          }
        }
      }
    }
  }
  if constexpr (kVals) {
    sum = wave_sum(sum);
    mnk = wave_min(mnk);
    mxk = wave_max(mxk);
  }
  if (lane == 0) {
    red[wid][0] = cnt;
    red[wid][1] = sum_bits(sum);
    red[wid][2] = mnk;
    red[wid][3] = mxk;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    // waves in order: the same geometry gives the same float sum
    uint64_t c = 0, lo = ~0ull, hi = 0;
    S s = 0;
    for (uint32_t k = 0; k < 4; ++k) {
      c += red[k][0];
      if constexpr (Tr<T>::flt) s += __longlong_as_double((long long)red[k][1]);
      else s += red[k][1];
      lo = umin64(lo, red[k][2]);
      hi = umax64(hi, red[k][3]);
    }
    uint64_t *out = slabs + (uint64_t)blockIdx.x * nacc_of(ops);
    uint32_t j = 0;
    if (ops & STROM_AGG_COUNT) out[j++] = c;
    if (ops & STROM_AGG_SUM) out[j++] = sum_bits(s);
    if (ops & STROM_AGG_MIN) out[j++] = lo;
    if (ops & STROM_AGG_MAX) out[j++] = hi;
  }
}

// ---------------------------------------------------------------- with key
// the key of row i as a slot candidate (signed types keep their sign: a
// negative dictionary index is malformed data, not a large slot)
__device__ __forceinline__ int64_t key_load(int kt, const void *p, uint64_t i) {
  switch (kt) {
    case STROM_COL_I8: return ((const int8_t *)p)[i];
    case STROM_COL_U8: return ((const uint8_t *)p)[i];
    case STROM_COL_I16: return ((const int16_t *)p)[i];
    case STROM_COL_U16: return ((const uint16_t *)p)[i];
    case STROM_COL_I32: return ((const int32_t *)p)[i];
    case STROM_COL_U32: return ((const uint32_t *)p)[i];
    case STROM_COL_I64: return ((const int64_t *)p)[i];
    case STROM_COL_U64: {
      const uint64_t v = ((const uint64_t *)p)[i];
      return v > (uint64_t)INT64_MAX ? -1 : (int64_t)v;
    }
    default: return (((const uint8_t *)p)[i >> 3] >> (i & 7)) & 1;   // STROM_COL_BOOL
  }
}

// position j of each accumulator array among the requested ones
struct AccPos {
  uint32_t cnt, sum, mn, mx, n;
};
__device__ __forceinline__ AccPos acc_pos(uint32_t ops) {
  AccPos p{0, 0, 0, 0, 0};
  if (ops & STROM_AGG_COUNT) p.cnt = p.n++;
  if (ops & STROM_AGG_SUM) p.sum = p.n++;
  if (ops & STROM_AGG_MIN) p.mn = p.n++;
  if (ops & STROM_AGG_MAX) p.mx = p.n++;
  return p;
}

// kind of accumulator array j: 0 count, 1 sum, 2 min, 3 max
__device__ __forceinline__ uint32_t acc_kind(uint32_t ops, uint32_t j) {
  uint32_t k = 0;
  for (uint32_t bit = 0; bit < 4; ++bit)
    if (ops & (1u << bit)) {
      if (k == j) return bit;
      ++k;
    }
  return 0;
}

template <bool FLT>
__device__ __forceinline__ uint64_t acc_comb(uint32_t kind, uint64_t a, uint64_t b) {
  if (kind == 2) return umin64(a, b);
  if (kind == 3) return umax64(a, b);
  if (FLT && kind == 1)
    return (uint64_t)__double_as_longlong(__longlong_as_double((long long)a) +
                                          __longlong_as_double((long long)b));
  return a + b;
}

// one row's (or one reduced wave's) contribution to slot `at` of the LDS set
template <typename T>
__device__ __forceinline__ void lds_update(uint64_t *acc, const AccPos &p, uint32_t ops,
                                           uint32_t stride, uint32_t at, uint64_t cnt,
                                           typename Tr<T>::sum_t sum, uint64_t mnk, uint64_t mxk) {
  typedef unsigned long long ull;
  if (ops & STROM_AGG_COUNT) atomicAdd((ull *)&acc[p.cnt * stride + at], (ull)cnt);
  if constexpr (!std::is_same<T, NoneT>::value) {
    if (ops & STROM_AGG_SUM) {
      if constexpr (Tr<T>::flt) unsafeAtomicAdd((double *)&acc[p.sum * stride + at], sum);
      else atomicAdd((ull *)&acc[p.sum * stride + at], (ull)sum);
    }
    // (~0, 0): no value that is not NaN — and no-ops as min / max operands
    if ((ops & STROM_AGG_MIN) && mnk != ~0ull) atomicMin((ull *)&acc[p.mn * stride + at], (ull)mnk);
    if ((ops & STROM_AGG_MAX) && mxk != 0) atomicMax((ull *)&acc[p.mx * stride + at], (ull)mxk);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void agg_keyed_kernel(const uint64_t *__restrict__ bm,
                                                        uint64_t nwords,
                                                        const strom_filter_batch *__restrict__ vt,
                                                        const strom_filter_batch *__restrict__ kt,
                                                        uint32_t nb, uint32_t ops, int key_type,
                                                        uint32_t G, uint32_t R,
                                                        uint64_t *__restrict__ slabs,
                                                        unsigned long long *__restrict__ bad_keys) {
  typedef typename Tr<T>::sum_t S;
  constexpr bool kVals = !std::is_same<T, NoneT>::value;
  extern __shared__ __attribute__((aligned(16))) uint64_t acc[];   // [array][slot][replica]
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const bool all = ops & STROM_AGG_ALL;
  const AccPos p = acc_pos(ops);
  const uint32_t stride = G * R, total = p.n * stride;
  for (uint32_t e = threadIdx.x; e < total; e += 256)
    acc[e] = acc_kind(ops, e / stride) == 2 ? ~0ull : 0;
  __syncthreads();
  const uint32_t rep = threadIdx.x & (R - 1);
  const int64_t nkeys = (int64_t)G - 1;
  uint32_t nbad = 0;
  // a run of words whose selected rows share one key: registers, as the
  // unkeyed walk (run_cnt is wave-uniform)
  bool run = false;
  uint32_t run_slot = 0;
  uint64_t run_cnt = 0, mnk = ~0ull, mxk = 0;
  S sum = 0;
  auto flush = [&]() {
    if constexpr (kVals) {
      sum = wave_sum(sum);
      mnk = wave_min(mnk);
      mxk = wave_max(mxk);
    }
    if (lane == 0 && run_cnt) lds_update<T>(acc, p, ops, stride, run_slot * R + rep, run_cnt, sum, mnk, mxk);
    run = false;
    run_cnt = 0;
    sum = 0;
    mnk = ~0ull;
    mxk = 0;
  };
  const uint64_t step = (uint64_t)gridDim.x * 4 * kU;
  for (uint64_t w0 = ((uint64_t)blockIdx.x * 4 + wid) * kU; w0 < nwords; w0 += step) {
    WordIn in[kU];
    S x[kU];
    int64_t kv[kU];
    uint64_t kvalid[kU];
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u) {
      in[u] = word_in(bm, nwords, w0 + u, vt, nb, all);
      x[u] = 0;
      kv[u] = 0;
      kvalid[u] = ~0ull;
      if (!in[u].sel) continue;
      const uint64_t i = in[u].k * 64 + lane;
      const strom_filter_batch &kb = kt[in[u].bi];
      if (kb.valid) kvalid[u] = ((const uint64_t *)kb.valid)[in[u].k];
      if ((in[u].sel >> lane) & 1) kv[u] = key_load(key_type, (const void *)kb.values, i);
      if constexpr (kVals)
        if ((in[u].use >> lane) & 1) x[u] = Tr<T>::widen(((const T *)vt[in[u].bi].values)[i]);
    }
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u) {
      if (!in[u].sel) continue;
      const bool sel = (in[u].sel >> lane) & 1;
      const bool knull = !((kvalid[u] >> lane) & 1);
      const bool bad = sel && !knull && (kv[u] < 0 || kv[u] >= nkeys);
      nbad += bad;
      const bool act = sel && !bad;
      const uint32_t slot = knull ? (uint32_t)nkeys : (uint32_t)kv[u];
      const uint64_t am = __ballot(act);
      if (!am) continue;
      const bool use = act && ((in[u].use >> lane) & 1);
      const uint32_t k0 = (uint32_t)__builtin_amdgcn_readfirstlane(
          __shfl((int)slot, (int)(__ffsll((unsigned long long)am) - 1), 64));
      if (!__ballot(act && slot != k0)) {
        if (run && run_slot != k0) flush();
        run = true;
        run_slot = k0;
        run_cnt += __popcll(__ballot(use));
        if constexpr (kVals) {
          if (use) {
            sum += x[u];
            if (!Tr<T>::nan(x[u])) {
              const uint64_t k = Tr<T>::key(x[u]);
              mnk = umin64(mnk, k);
              mxk = umax64(mxk, k);
            }
          }
        }
      } else if (use) {
        uint64_t lo = ~0ull, hi = 0;
        if constexpr (kVals)
          if (!Tr<T>::nan(x[u])) lo = hi = Tr<T>::key(x[u]);
        lds_update<T>(acc, p, ops, stride, slot * R + rep, 1, x[u], lo, hi);
      }
    }
  }
  if (run) flush();
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nbad += __shfl_xor(nbad, o, 64);
  if (lane == 0 && nbad && bad_keys) atomicAdd(bad_keys, (unsigned long long)nbad);
  __syncthreads();
  // the slab: replicas folded in a fixed (rotated: no bank conflict) order
  uint64_t *out = slabs + (uint64_t)blockIdx.x * p.n * G;
  for (uint32_t e = threadIdx.x; e < p.n * G; e += 256) {
    const uint32_t kind = acc_kind(ops, e / G);
    uint64_t v = acc[e * R + (e & (R - 1))];
    for (uint32_t r = 1; r < R; ++r)
      v = acc_comb<Tr<T>::flt>(kind, v, acc[e * R + ((e + r) & (R - 1))]);
    out[e] = v;
  }
}

// ------------------------------------------------------------------ reduce
// entry[e] = entry[e] (+) slab_0[e] (+) slab_1[e] ...: L lanes per element,
// lane s folds slabs s, s + L, ... in order, then a fixed xor tree
template <bool FLT>
__global__ __launch_bounds__(256) void agg_reduce_kernel(const uint64_t *__restrict__ slabs,
                                                         uint32_t nslabs, uint32_t nelem,
                                                         uint32_t G, uint32_t ops, uint32_t L,
                                                         uint64_t *__restrict__ entry) {
  const uint32_t t = blockIdx.x * 256 + threadIdx.x;
  const uint32_t e = t / L, s = t % L;
  const bool live = e < nelem;
  const uint32_t kind = acc_kind(ops, live ? e / G : 0);
  uint64_t v = kind == 2 ? ~0ull : 0;
  if (live)
    for (uint32_t b = s; b < nslabs; b += L) v = acc_comb<FLT>(kind, v, slabs[(uint64_t)b * nelem + e]);
  for (uint32_t o = L >> 1; o > 0; o >>= 1)
    v = acc_comb<FLT>(kind, v, (uint64_t)__shfl_xor((unsigned long long)v, (int)o, 64));
  if (live && s == 0) entry[e] = acc_comb<FLT>(kind, entry[e], v);
}

__global__ __launch_bounds__(256) void agg_init_kernel(uint64_t *__restrict__ entry, uint32_t nelem,
                                                       uint32_t G, uint32_t ops) {
  const uint32_t e = blockIdx.x * 256 + threadIdx.x;
  if (e < nelem) entry[e] = acc_kind(ops, e / G) == 2 ? ~0ull : 0;
}

uint32_t host_nacc(uint32_t ops) { return (uint32_t)__builtin_popcount(ops & 15u); }

// workgroups of a launch: each walks at least one trip of its four waves
// (16 words), and at least 16 rows per accumulator word it flushes (the slab
// traffic stays a fraction of the column's)
uint32_t agg_grid(uint64_t nwords, uint32_t ops, uint32_t nslots) {
  uint64_t per = (uint64_t)host_nacc(ops) * nslots / 4;
  if (per < 4 * kU) per = 4 * kU;
  const uint64_t g = (nwords + per - 1) / per;
  return (uint32_t)(g > kMaxGrid ? kMaxGrid : (g ? g : 1));
}

template <typename T>
int launch_agg(uint32_t ops, const uint64_t *bm, uint64_t nwords, const strom_filter_batch *vt,
               const strom_filter_batch *kt, int key_type, uint32_t G, uint32_t nb,
               uint64_t *slabs, uint64_t *bad, hipStream_t st) {
  const uint32_t grid = agg_grid(nwords, ops, G);
  if (!kt) {
    hipLaunchKernelGGL(agg_flat_kernel<T>, dim3(grid), dim3(256), 0, st, bm, nwords, vt, nb, ops,
                       slabs);
  } else {
    const uint32_t words = host_nacc(ops) * G;
    uint32_t R = 256;
    while (R > 1 && (uint64_t)words * R * 8 > STROM_AGG_LDS_BYTES) R >>= 1;
    hipLaunchKernelGGL(agg_keyed_kernel<T>, dim3(grid), dim3(256), (size_t)words * R * 8, st, bm,
                       nwords, vt, kt, nb, ops, key_type, G, R, slabs, (unsigned long long *)bad);
  }
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // namespace

extern "C" uint32_t strom_column_agg_grid(uint64_t nwords, uint32_t ops, uint32_t nslots) {
  return agg_grid(nwords, ops, nslots ? nslots : 1);
}

extern "C" int strom_column_agg_init(uint32_t ops, uint32_t nslots, uint64_t *d_acc, void *stream) {
  const uint32_t n = host_nacc(ops);
  if (!n || !nslots || !d_acc || ((uintptr_t)d_acc & 7)) return -22;
  const uint32_t nelem = n * nslots;
  hipLaunchKernelGGL(agg_init_kernel, dim3((nelem + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                     d_acc, nelem, nslots, ops);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int strom_column_agg(int type, uint32_t ops, const uint64_t *d_bitmap, uint64_t nwords,
                                const strom_filter_batch *d_vals, const strom_filter_batch *d_keys,
                                int key_type, uint32_t nslots, uint32_t nbatches, uint64_t *d_slabs,
                                uint64_t slab_words, uint64_t *d_bad_keys, void *stream) {
  const uint32_t n = host_nacc(ops);
  if (!n || !nslots || !nbatches || !d_bitmap || !d_vals || !d_slabs || ((uintptr_t)d_slabs & 7))
    return -22;
  if (type == STROM_COL_NONE && (ops & (STROM_AGG_SUM | STROM_AGG_MIN | STROM_AGG_MAX))) return -22;
  if (d_keys) {
    if (nslots < 2) return -22;
    if (key_type != STROM_COL_BOOL && (key_type < STROM_COL_I32 || key_type > STROM_COL_U64 ||
                                       key_type == STROM_COL_F32 || key_type == STROM_COL_F64))
      return -22;
  } else if (nslots != 1) {
    return -22;
  }
  if ((uint64_t)n * nslots * 8 > STROM_AGG_LDS_BYTES) return -7;
  if (slab_words < (uint64_t)agg_grid(nwords, ops, nslots) * n * nslots) return -22;
  hipStream_t st = (hipStream_t)stream;
#define AGG(T) launch_agg<T>(ops, d_bitmap, nwords, d_vals, d_keys, key_type, nslots, nbatches, \
                             d_slabs, d_bad_keys, st)
  switch (type) {
    case STROM_COL_NONE: return AGG(NoneT);
    case STROM_COL_I8: return AGG(int8_t);
    case STROM_COL_I16: return AGG(int16_t);
    case STROM_COL_I32: return AGG(int32_t);
    case STROM_COL_I64: return AGG(int64_t);
    case STROM_COL_U8: return AGG(uint8_t);
    case STROM_COL_U16: return AGG(uint16_t);
    case STROM_COL_U32: return AGG(uint32_t);
    case STROM_COL_U64: return AGG(uint64_t);
    case STROM_COL_F32: return AGG(float);
    case STROM_COL_F64: return AGG(double);
    default: return -22;
  }
#undef AGG
}

extern "C" int strom_column_agg_reduce(int type, uint32_t ops, uint32_t nslots,
                                       const uint64_t *d_slabs, uint32_t nslabs, uint64_t *d_acc,
                                       void *stream) {
  const uint32_t n = host_nacc(ops);
  if (!n || !nslots || !d_slabs || !d_acc || ((uintptr_t)d_acc & 7)) return -22;
  if (!nslabs) return 0;
  const uint32_t nelem = n * nslots;
  uint32_t L = 64;
  while (L > 1 && (uint64_t)nelem * L > 16384) L >>= 1;
  const uint32_t grid = (uint32_t)(((uint64_t)nelem * L + 255) / 256);
  hipStream_t st = (hipStream_t)stream;
  if (type == STROM_COL_F32 || type == STROM_COL_F64)
    hipLaunchKernelGGL(agg_reduce_kernel<true>, dim3(grid), dim3(256), 0, st, d_slabs, nslabs, nelem,
                       nslots, ops, L, d_acc);
  else
    hipLaunchKernelGGL(agg_reduce_kernel<false>, dim3(grid), dim3(256), 0, st, d_slabs, nslabs,
                       nelem, nslots, ops, L, d_acc);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

// Every entry of a query over one group in one call (the host's time per
// group is on the scan's read path): entry i's launch writes e[i].slabs
// (strom_column_agg_grid * popcount(ops) * nslots words); malformed keys are
// counted once, by entry 0's launch.
extern "C" int strom_column_agg_many(const strom_agg_entry *e, uint32_t n, const uint64_t *d_bitmap,
                                     uint64_t nwords, const strom_filter_batch *d_keys,
                                     int key_type, uint32_t nslots, uint32_t nbatches,
                                     uint64_t *d_bad_keys, void *stream) {
  if (!e) return -22;
  for (uint32_t i = 0; i < n; ++i) {
    const uint64_t words = (uint64_t)agg_grid(nwords, e[i].ops, nslots ? nslots : 1) *
                           host_nacc(e[i].ops) * nslots;
    const int rc = strom_column_agg(e[i].type, e[i].ops, d_bitmap, nwords,
                                    (const strom_filter_batch *)e[i].vals, d_keys, key_type, nslots,
                                    nbatches, (uint64_t *)e[i].slabs, words,
                                    i == 0 ? d_bad_keys : nullptr, stream);
    if (rc) return rc;
  }
  return 0;
}

extern "C" int strom_column_agg_reduce_many(const strom_agg_entry *e, uint32_t n, uint32_t nslots,
                                            uint64_t nwords, void *stream) {
  if (!e) return -22;
  for (uint32_t i = 0; i < n; ++i) {
    const int rc = strom_column_agg_reduce(e[i].type, e[i].ops, nslots, (const uint64_t *)e[i].slabs,
                                           agg_grid(nwords, e[i].ops, nslots ? nslots : 1),
                                           (uint64_t *)e[i].acc, stream);
    if (rc) return rc;
  }
  return 0;
}
