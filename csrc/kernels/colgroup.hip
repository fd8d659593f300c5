// colgroup.hip — hash GROUP BY on an integer key column of a columnar scan
// (PG-Strom's GpuPreAgg is a hash aggregation; colagg.hip is its small-domain
// form, whose accumulators fit LDS).
//
// Table: STROM_GROUP_HDR_WORDS header words and `capacity` 64-bit key words
// (a power of two >= 2 * groups), open addressing with linear probing from
// fmix64(key) & (capacity - 1) — the hash of coljoin.hip.  A free slot holds
// STROM_JOIN_EMPTY; that bit pattern is a legal key all the same and owns the
// reserved code capacity + 1, as the null keys own code capacity.  Every
// accumulator array is capacity + 2 elements, indexed by code, and is set to
// its identity by the init launch, before any launch can see a slot: claiming
// a slot is the CAS on its key word and nothing else.
//
// Codes (find-or-insert): the walk of join_probe_kernel — one wave per
// 64-row bitmap word, kU words per trip, the home slots loaded before the
// first compare.  A plain load that still sees a slot free is settled by the
// CAS (a key word changes once, from free to its key, so a stale load can
// only say "free").  The row's code goes to an int32 buffer that the
// accumulate launches read as their key column.  GROUP BY a, b, ... takes the
// same walk (group_codes_multi_kernel): each lane packs its row's components
// into one key word first.
//
// Accumulate: the walk of agg_keyed_kernel with the accumulators in HBM,
// updated with device-scope atomics (u64 add / min / max, f64 add).  There
// are no slabs: a slab of `capacity` elements per workgroup is not affordable,
// so unlike colagg.hip the workgroups do meet in global float atomics and a
// float sum depends on arrival order.  A run of words whose selected rows
// carry one code is summed in registers and flushed with one wave reduction
// and one set of atomics: sorted or clustered keys never put 64 lanes on one
// address.  In a word of mixed codes the rows that share the first selected
// row's code join that run too (`combine`): a hot key interleaved with others
// stays in registers from word to word instead of serialising every
// workgroup on one address.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "strom/strom.h"

namespace {

constexpr uint32_t kU = 4;          // words per wave and trip (as colfilter.hip)
constexpr uint32_t kMaxGrid = 8192;
constexpr uint64_t kEmpty = STROM_JOIN_EMPTY;
constexpr uint32_t kHdr = STROM_GROUP_HDR_WORDS;
constexpr uint64_t kSign = 1ull << 63;
typedef unsigned long long ull;

struct NoneT {};                    // STROM_COL_NONE: validity only

// murmur3's 64-bit finalizer (coljoin.hip, ops/coljoin.hash64)
__device__ __forceinline__ uint64_t fmix64(uint64_t k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return k;
}

__device__ __forceinline__ uint32_t batch_of(const strom_filter_batch *b, uint32_t nb, uint64_t w) {
  uint32_t lo = 0, hi = nb;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (b[mid].word_base <= w) lo = mid;
    else hi = mid;
  }
  return lo;
}

// rows of batch word k that exist
__device__ __forceinline__ uint64_t row_mask(const strom_filter_batch &b, uint64_t k) {
  if (k * 64 >= b.nrows) return 0;
  const uint64_t rem = b.nrows - k * 64;
  return rem >= 64 ? ~0ull : (1ull << rem) - 1;
}

__device__ __forceinline__ uint64_t umin64(uint64_t a, uint64_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint64_t umax64(uint64_t a, uint64_t b) { return a > b ? a : b; }

__host__ __device__ __forceinline__ uint32_t nacc_of(uint32_t ops) {
  return (uint32_t)__builtin_popcount(ops & 15u);
}

// -------------------------------------------------------------------- init
__global__ __launch_bounds__(256) void group_init_table_kernel(uint64_t *__restrict__ table,
                                                               uint64_t capacity) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t step = (uint64_t)gridDim.x * 256;
  if (i < kHdr) table[i] = i == STROM_GROUP_H_CAPACITY ? capacity : 0;
  for (uint64_t s = i; s < capacity; s += step) table[kHdr + s] = kEmpty;
}

// one entry's arrays: counts and sums 0, min keys ~0, max keys 0 (colagg.hip)
__global__ __launch_bounds__(256) void group_init_acc_kernel(uint64_t *__restrict__ acc,
                                                             uint64_t stride, uint32_t ops) {
  const uint64_t step = (uint64_t)gridDim.x * 256;
  uint32_t j = 0;
  for (uint32_t bit = 0; bit < 4; ++bit) {
    if (!(ops & (1u << bit))) continue;
    const uint64_t v = bit == 2 ? ~0ull : 0;
    uint64_t *a = acc + (uint64_t)j * stride;
    for (uint64_t s = (uint64_t)blockIdx.x * 256 + threadIdx.x; s < stride; s += step) a[s] = v;
    ++j;
  }
}

// ------------------------------------------------------------------- codes
// the key of a row as its 64-bit pattern: signed types sign-extended,
// unsigned ones zero-extended (one column type: the mapping is one to one)
template <typename T> __device__ __forceinline__ uint64_t widen_key(T x) {
  if constexpr (std::is_signed<T>::value) return (uint64_t)(int64_t)x;
  else return (uint64_t)x;
}

template <typename T>
__global__ __launch_bounds__(256) void group_codes_kernel(uint64_t *table, uint64_t capacity,
                                                          const strom_filter_batch *__restrict__ kt,
                                                          uint32_t nb, uint64_t nwords,
                                                          const uint64_t *src, uint64_t *dst,
                                                          const strom_filter_batch *__restrict__ ct) {
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint64_t mask = capacity - 1;
  uint64_t *slots = table + kHdr;
  uint32_t nins = 0, nover = 0;                       // wave-uniform
  const uint64_t step = (uint64_t)gridDim.x * 4 * kU;
  for (uint64_t w0 = ((uint64_t)blockIdx.x * 4 + wid) * kU; w0 < nwords; w0 += step) {
    uint64_t raw[kU], sel[kU], key[kU], at[kU], bk[kU], e[kU];
    uint32_t bi[kU];
    bool act[kU];                   // this lane looks for a slot
    int32_t code[kU];
    // pass 1: the source word, the key, the home slot's load
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u) {
      const uint64_t w = w0 + u;
      raw[u] = 0;
      sel[u] = 0;
      key[u] = 0;
      at[u] = 0;
      bk[u] = 0;
      bi[u] = 0;
      act[u] = false;
      code[u] = 0;
      e[u] = kEmpty;
      if (w >= nwords) continue;
      const uint64_t word = src[w];                    // uniform load, one per wave
      if (!word) continue;
      raw[u] = word;
      bi[u] = batch_of(kt, nb, w);
      const strom_filter_batch &b = kt[bi[u]];
      bk[u] = w - b.word_base;
      sel[u] = word & row_mask(b, bk[u]);
      if (!((sel[u] >> lane) & 1)) continue;
      if (b.valid && !((((const uint64_t *)b.valid)[bk[u]] >> lane) & 1)) {
        code[u] = (int32_t)capacity;                   // the null keys' group
        continue;
      }
      key[u] = widen_key<T>(((const T *)b.values)[bk[u] * 64 + lane]);
      if (key[u] == kEmpty) {
        // the one key the slots cannot hold: a flag in the header
        code[u] = (int32_t)(capacity + 1);
        if (!table[STROM_GROUP_H_HAS_EMPTY] &&
            atomicCAS((ull *)&table[STROM_GROUP_H_HAS_EMPTY], 0ull, 1ull) == 0ull)
          atomicAdd((ull *)&table[STROM_GROUP_H_NKEYS], 1ull);      // once per table
        continue;
      }
      act[u] = true;
      at[u] = fmix64(key[u]) & mask;
      e[u] = slots[at[u]];
    }
    // pass 2: compare, claim a free slot, walk on while it holds another key
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u) {
      const uint64_t w = w0 + u;
      if (w >= nwords) break;
      uint64_t word = sel[u];
      if (sel[u]) {
        bool go = act[u], ins = false, over = false;
        // at most `capacity` slots are looked at, whatever the arguments
        for (uint64_t d = 0;; ++d) {
          if (go) {
            uint64_t cur = e[u];
            if (cur == kEmpty) {
              cur = atomicCAS((ull *)&slots[at[u]], (ull)kEmpty, (ull)key[u]);
              if (cur == kEmpty) {
                ins = true;
                cur = key[u];
              }
            }
            if (cur == key[u]) {
              code[u] = (int32_t)at[u];
              go = false;
            } else if (d + 1 >= capacity) {
              over = true;
              go = false;
            }
          }
          if (!__ballot(go)) break;
          if (go) {
            at[u] = (at[u] + 1) & mask;
            e[u] = slots[at[u]];
          }
        }
        nins += __popcll(__ballot(ins));
        const uint64_t om = __ballot(over);
        nover += __popcll(om);
        word &= ~om;                                   // no code: not accumulated
        if ((sel[u] >> lane) & 1)
          ((int32_t *)ct[bi[u]].values)[bk[u] * 64 + lane] = code[u];
      }
      // in place, a word that stays as it is (a zero one above all) is not stored
      if (lane == 0 && (dst != src || word != raw[u])) dst[w] = word;
    }
  }
  // the counters once per wave
  if (lane == 0) {
    if (nins) atomicAdd((ull *)&table[STROM_GROUP_H_NKEYS], (ull)nins);
    if (nover) atomicAdd((ull *)&table[STROM_GROUP_H_OVERFLOW], (ull)nover);
  }
}

template <typename T>
int launch_codes(uint64_t *table, uint64_t capacity, const strom_filter_batch *kt, uint32_t nb,
                 uint64_t nwords, const uint64_t *src, uint64_t *dst,
                 const strom_filter_batch *ct, hipStream_t st) {
  const uint64_t g = (nwords + 4 * kU - 1) / (4 * kU);
  const uint32_t grid = (uint32_t)(g > kMaxGrid ? kMaxGrid : (g ? g : 1));
  hipLaunchKernelGGL(group_codes_kernel<T>, dim3(grid), dim3(256), 0, st, table, capacity, kt, nb,
                     nwords, src, dst, ct);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

// ------------------------------------------------- codes, composite keys
// Up to STROM_GROUP_MAX_KEYS components packed into the one key word of the
// table above (strom.h: component i's field is bits (+ 1 when nullable) wide
// at `shift`, the first component in the most significant used bits, a signed
// value stored as v + 2^(bits - 1), a null as the field's top bit alone).
// Unsigned order of the word is lexicographic order of the tuples, so the
// table, its single CAS and everything behind it stay as they are.

// the value at row i of a column of storage type `type`, by value (signed
// types sign-extended).  `type` is a kernel argument: the switch is uniform.
__device__ __forceinline__ uint64_t load_wide(uint32_t type, const void *p, uint64_t i) {
  switch (type) {
    case STROM_COL_I8: return (uint64_t)(int64_t)((const int8_t *)p)[i];
    case STROM_COL_I16: return (uint64_t)(int64_t)((const int16_t *)p)[i];
    case STROM_COL_I32: return (uint64_t)(int64_t)((const int32_t *)p)[i];
    case STROM_COL_U8: return ((const uint8_t *)p)[i];
    case STROM_COL_U16: return ((const uint16_t *)p)[i];
    case STROM_COL_U32: return ((const uint32_t *)p)[i];
    default: return ((const uint64_t *)p)[i];          // I64, U64
  }
}

__host__ __device__ __forceinline__ bool key_signed(uint32_t type) {
  return type == STROM_COL_I8 || type == STROM_COL_I16 || type == STROM_COL_I32 ||
         type == STROM_COL_I64;
}

template <int NK>
__global__ __launch_bounds__(256) void group_codes_multi_kernel(
    strom_group_keys ks, uint64_t *table, uint64_t capacity,
    const strom_filter_batch *__restrict__ kt, uint32_t nb, uint64_t nwords, const uint64_t *src,
    uint64_t *dst, const strom_filter_batch *__restrict__ ct) {
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint64_t mask = capacity - 1;
  uint64_t *slots = table + kHdr;
  uint32_t nins = 0, nover = 0, nrange[NK];           // wave-uniform
#pragma unroll
  for (int i = 0; i < NK; ++i) nrange[i] = 0;
  const uint64_t step = (uint64_t)gridDim.x * 4 * kU;
  for (uint64_t w0 = ((uint64_t)blockIdx.x * 4 + wid) * kU; w0 < nwords; w0 += step) {
    uint64_t raw[kU], sel[kU], key[kU], at[kU], bk[kU], e[kU];
    uint32_t bi[kU];
    int32_t bad[kU];                // the first component that does not fit, or -1
    bool act[kU];
    int32_t code[kU];
    // pass 1: the source word, every component's value (read before any code
    // is stored: a component may live in the code buffer), the packed key,
    // the home slot's load
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u) {
      const uint64_t w = w0 + u;
      raw[u] = 0;
      sel[u] = 0;
      key[u] = 0;
      at[u] = 0;
      bk[u] = 0;
      bi[u] = 0;
      bad[u] = -1;
      act[u] = false;
      code[u] = 0;
      e[u] = kEmpty;
      if (w >= nwords) continue;
      const uint64_t word = src[w];                    // uniform load, one per wave
      if (!word) continue;
      raw[u] = word;
      // the components' tables describe the same batches: one search
      bi[u] = batch_of(kt, nb, w);
      const strom_filter_batch &b0 = kt[bi[u]];
      bk[u] = w - b0.word_base;
      sel[u] = word & row_mask(b0, bk[u]);
      if (!((sel[u] >> lane) & 1)) continue;
      uint64_t packed = 0;
#pragma unroll
      for (int i = 0; i < NK; ++i) {
        const strom_group_key &kd = ks.k[i];
        const strom_filter_batch &b = kt[(uint64_t)i * nb + bi[u]];
        uint64_t f;
        bool fits;
        if (b.valid && !((((const uint64_t *)b.valid)[bk[u]] >> lane) & 1)) {
          // a null where none was declared has no field value
          fits = kd.nullable != 0;
          f = 1ull << (kd.bits & 63);
        } else {
          f = load_wide(kd.type, (const void *)b.values, bk[u] * 64 + lane);
          if (key_signed(kd.type)) f += 1ull << (kd.bits - 1);
          fits = kd.bits >= 64 || !(f >> kd.bits);
        }
        if (!fits && bad[u] < 0) bad[u] = i;
        packed |= f << kd.shift;
      }
      if (bad[u] >= 0) continue;                       // no code; cleared in pass 2
      key[u] = packed;
      if (key[u] == kEmpty) {
        // the one key the slots cannot hold: a flag in the header
        code[u] = (int32_t)(capacity + 1);
        if (!table[STROM_GROUP_H_HAS_EMPTY] &&
            atomicCAS((ull *)&table[STROM_GROUP_H_HAS_EMPTY], 0ull, 1ull) == 0ull)
          atomicAdd((ull *)&table[STROM_GROUP_H_NKEYS], 1ull);      // once per table
        continue;
      }
      act[u] = true;
      at[u] = fmix64(key[u]) & mask;
      e[u] = slots[at[u]];
    }
    // pass 2: compare, claim a free slot, walk on while it holds another key
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u) {
      const uint64_t w = w0 + u;
      if (w >= nwords) break;
      uint64_t word = sel[u];
      if (sel[u]) {
        bool go = act[u], ins = false, over = false;
        // at most `capacity` slots are looked at, whatever the arguments
        for (uint64_t d = 0;; ++d) {
          if (go) {
            uint64_t cur = e[u];
            if (cur == kEmpty) {
              cur = atomicCAS((ull *)&slots[at[u]], (ull)kEmpty, (ull)key[u]);
              if (cur == kEmpty) {
                ins = true;
                cur = key[u];
              }
            }
            if (cur == key[u]) {
              code[u] = (int32_t)at[u];
              go = false;
            } else if (d + 1 >= capacity) {
              over = true;
              go = false;
            }
          }
          if (!__ballot(go)) break;
          if (go) {
            at[u] = (at[u] + 1) & mask;
            e[u] = slots[at[u]];
          }
        }
        nins += __popcll(__ballot(ins));
        const uint64_t om = __ballot(over);
        nover += __popcll(om);
        word &= ~om;                                   // no code: not accumulated
#pragma unroll
        for (int i = 0; i < NK; ++i) {
          const uint64_t rm = __ballot(bad[u] == i);
          nrange[i] += __popcll(rm);
          word &= ~rm;
        }
        if ((sel[u] >> lane) & 1)
          ((int32_t *)ct[bi[u]].values)[bk[u] * 64 + lane] = code[u];
      }
      // in place, a word that stays as it is (a zero one above all) is not stored
      if (lane == 0 && (dst != src || word != raw[u])) dst[w] = word;
    }
  }
  // the counters once per wave
  if (lane == 0) {
    if (nins) atomicAdd((ull *)&table[STROM_GROUP_H_NKEYS], (ull)nins);
    if (nover) atomicAdd((ull *)&table[STROM_GROUP_H_OVERFLOW], (ull)nover);
#pragma unroll
    for (int i = 0; i < NK; ++i)
      if (nrange[i]) atomicAdd((ull *)&table[STROM_GROUP_H_RANGE + i], (ull)nrange[i]);
  }
}

template <int NK>
int launch_codes_multi(const strom_group_keys &ks, uint64_t *table, uint64_t capacity,
                       const strom_filter_batch *kt, uint32_t nb, uint64_t nwords,
                       const uint64_t *src, uint64_t *dst, const strom_filter_batch *ct,
                       hipStream_t st) {
  const uint64_t g = (nwords + 4 * kU - 1) / (4 * kU);
  const uint32_t grid = (uint32_t)(g > kMaxGrid ? kMaxGrid : (g ? g : 1));
  hipLaunchKernelGGL(group_codes_multi_kernel<NK>, dim3(grid), dim3(256), 0, st, ks, table,
                     capacity, kt, nb, nwords, src, dst, ct);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

// -------------------------------------------------------------- accumulate
// value traits: the sum's type, the widened value, its order-preserving key
// (colagg.hip)
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

template <typename S> __device__ __forceinline__ S wave_sum(S v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ uint64_t wave_min(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = umin64(v, (uint64_t)__shfl_xor((ull)v, o, 64));
  return v;
}
__device__ __forceinline__ uint64_t wave_max(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = umax64(v, (uint64_t)__shfl_xor((ull)v, o, 64));
  return v;
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

// one row's (or one reduced wave's) contribution to row `at` of the entry
template <typename T>
__device__ __forceinline__ void hbm_update(uint64_t *acc, const AccPos &p, uint32_t ops,
                                           uint64_t stride, uint64_t at, uint64_t cnt,
                                           typename Tr<T>::sum_t sum, uint64_t mnk, uint64_t mxk) {
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

template <typename T>
__global__ __launch_bounds__(256) void group_agg_kernel(const uint64_t *__restrict__ bm,
                                                        uint64_t nwords,
                                                        const strom_filter_batch *__restrict__ vt,
                                                        const strom_filter_batch *__restrict__ ct,
                                                        uint32_t nb, uint32_t ops,
                                                        uint64_t *__restrict__ acc, uint64_t stride,
                                                        int combine) {
  typedef typename Tr<T>::sum_t S;
  constexpr bool kVals = !std::is_same<T, NoneT>::value;
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const bool all = ops & STROM_AGG_ALL;
  const AccPos p = acc_pos(ops);
  // a run of words whose selected rows share one code: registers, as the
  // unkeyed walk of colagg.hip (run_cnt is wave-uniform)
  bool run = false;
  uint32_t run_code = 0;
  uint64_t run_cnt = 0, mnk = ~0ull, mxk = 0;
  S sum = 0;
  auto flush = [&]() {
    if constexpr (kVals) {
      sum = wave_sum(sum);
      mnk = wave_min(mnk);
      mxk = wave_max(mxk);
    }
    if (lane == 0 && run_cnt) hbm_update<T>(acc, p, ops, stride, run_code, run_cnt, sum, mnk, mxk);
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
    uint32_t cv[kU];
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u) {
      in[u] = word_in(bm, nwords, w0 + u, vt, nb, all);
      x[u] = 0;
      cv[u] = 0;
      if (!in[u].sel) continue;
      const uint64_t i = in[u].k * 64 + lane;
      if ((in[u].sel >> lane) & 1) cv[u] = (uint32_t)((const int32_t *)ct[in[u].bi].values)[i];
      if constexpr (kVals)
        if ((in[u].use >> lane) & 1) x[u] = Tr<T>::widen(((const T *)vt[in[u].bi].values)[i]);
    }
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u) {
      if (!in[u].sel) continue;
      // a code outside the arrays (never written by the codes launch) is not followed
      const bool act = ((in[u].sel >> lane) & 1) && cv[u] < stride;
      const uint64_t am = __ballot(act);
      if (!am) continue;
      const bool use = act && ((in[u].use >> lane) & 1);
      const uint32_t k0 = (uint32_t)__builtin_amdgcn_readfirstlane(
          __shfl((int)cv[u], (int)(__ffsll((ull)am) - 1), 64));
      const uint64_t same = __ballot(act && cv[u] == k0);
      if (same == am) {
        if (run && run_code != k0) flush();
        run = true;
        run_code = k0;
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
        continue;
      }
      uint64_t lo = ~0ull, hi = 0;
      if constexpr (kVals)
        if (use && !Tr<T>::nan(x[u])) lo = hi = Tr<T>::key(x[u]);
      bool single = use;
      if (combine && __popcll(same) > 1) {
        // the rows that carry the first selected row's code join the run in
        // registers (the hot key of a skewed column stays there from word to
        // word: profiles/r9/hashagg/SUMMARY.md); the others add on their own
        if (run && run_code != k0) flush();
        run = true;
        run_code = k0;
        const bool mine = use && cv[u] == k0;
        run_cnt += __popcll(__ballot(mine));
        if constexpr (kVals) {
          if (mine) {
            sum += x[u];
            mnk = umin64(mnk, lo);
            mxk = umax64(mxk, hi);
          }
        }
        single = use && cv[u] != k0;
      }
      if (single) hbm_update<T>(acc, p, ops, stride, cv[u], 1, x[u], lo, hi);
    }
  }
  if (run) flush();
}

template <typename T>
int launch_group_agg(uint32_t ops, const uint64_t *bm, uint64_t nwords, const strom_filter_batch *vt,
                     const strom_filter_batch *ct, uint32_t nb, uint64_t *acc, uint64_t stride,
                     int combine, hipStream_t st) {
  const uint64_t g = (nwords + 4 * kU - 1) / (4 * kU);
  const uint32_t grid = (uint32_t)(g > kMaxGrid ? kMaxGrid : (g ? g : 1));
  hipLaunchKernelGGL(group_agg_kernel<T>, dim3(grid), dim3(256), 0, st, bm, nwords, vt, ct, nb, ops,
                     acc, stride, combine);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

bool pow2(uint64_t x) { return x && !(x & (x - 1)); }
bool cap_ok(uint64_t c) { return pow2(c) && c >= 2 && c <= STROM_GROUP_MAX_CAPACITY; }

}  // namespace

extern "C" uint64_t strom_group_capacity(uint64_t groups) {
  uint64_t c = 2;
  while (c < 2 * groups) c <<= 1;
  return c;
}

extern "C" int strom_group_init(uint64_t *d_table, uint64_t capacity, const strom_agg_entry *e,
                                uint32_t n, void *stream) {
  if (!d_table || ((uintptr_t)d_table & 7) || !cap_ok(capacity) || (n && !e)) return -22;
  for (uint32_t i = 0; i < n; ++i)
    if (!nacc_of(e[i].ops) || !e[i].acc || (e[i].acc & 7)) return -22;
  hipStream_t st = (hipStream_t)stream;
  const uint64_t stride = capacity + 2;
  const uint64_t g = (stride + 255) / 256;
  const uint32_t grid = (uint32_t)(g > kMaxGrid ? kMaxGrid : g);
  hipLaunchKernelGGL(group_init_table_kernel, dim3(grid), dim3(256), 0, st, d_table, capacity);
  if (hipGetLastError() != hipSuccess) return -5;
  for (uint32_t i = 0; i < n; ++i) {
    hipLaunchKernelGGL(group_init_acc_kernel, dim3(grid), dim3(256), 0, st, (uint64_t *)e[i].acc,
                       stride, e[i].ops);
    if (hipGetLastError() != hipSuccess) return -5;
  }
  return 0;
}

extern "C" int strom_group_codes(int type, uint64_t *d_table, uint64_t capacity,
                                 const strom_filter_batch *d_keys, uint32_t nbatches,
                                 uint64_t nwords, const uint64_t *d_src, uint64_t *d_dst,
                                 const strom_filter_batch *d_codes, void *stream) {
  if (!d_table || ((uintptr_t)d_table & 7) || !cap_ok(capacity)) return -22;
  if (!d_keys || !d_codes || !nbatches || !d_src || !d_dst || ((uintptr_t)d_src & 7) ||
      ((uintptr_t)d_dst & 7))
    return -22;
  if (!nwords) return 0;
  hipStream_t st = (hipStream_t)stream;
#define CODES(T) launch_codes<T>(d_table, capacity, d_keys, nbatches, nwords, d_src, d_dst, \
                                 d_codes, st)
  switch (type) {
    case STROM_COL_I8: return CODES(int8_t);
    case STROM_COL_I16: return CODES(int16_t);
    case STROM_COL_I32: return CODES(int32_t);
    case STROM_COL_I64: return CODES(int64_t);
    case STROM_COL_U8: return CODES(uint8_t);
    case STROM_COL_U16: return CODES(uint16_t);
    case STROM_COL_U32: return CODES(uint32_t);
    case STROM_COL_U64: return CODES(uint64_t);
    default: return -22;        // floats, strings, bool, decimal: no integer key
  }
#undef CODES
}

namespace {

uint32_t key_storage_bits(uint32_t type) {
  switch (type) {
    case STROM_COL_I8: case STROM_COL_U8: return 8;
    case STROM_COL_I16: case STROM_COL_U16: return 16;
    case STROM_COL_I32: case STROM_COL_U32: return 32;
    case STROM_COL_I64: case STROM_COL_U64: return 64;
    default: return 0;          // floats, strings, bool, decimal: no integer key
  }
}

// fields inside the word, the first component on top, none overlapping
bool keys_ok(const strom_group_keys &ks) {
  if (ks.nkeys < 1 || ks.nkeys > STROM_GROUP_MAX_KEYS) return false;
  uint32_t top = 64;            // the bits below `top` are still free
  for (uint32_t i = 0; i < ks.nkeys; ++i) {
    const strom_group_key &k = ks.k[i];
    const uint32_t sb = key_storage_bits(k.type);
    if (!sb || k.bits < 1 || k.bits > sb || k.nullable > 1) return false;
    const uint32_t width = k.bits + k.nullable;
    if (width > 64 || k.shift > 64 - width || k.shift + width > top) return false;
    top = k.shift;
  }
  return true;
}

}  // namespace

extern "C" int strom_group_codes_multi(struct strom_group_keys keys, uint64_t *d_table,
                                       uint64_t capacity, const strom_filter_batch *d_keys,
                                       uint32_t nbatches, uint64_t nwords, const uint64_t *d_src,
                                       uint64_t *d_dst, const strom_filter_batch *d_codes,
                                       void *stream) {
  if (!d_table || ((uintptr_t)d_table & 7) || !cap_ok(capacity) || !keys_ok(keys)) return -22;
  if (!d_keys || !d_codes || !nbatches || !d_src || !d_dst || ((uintptr_t)d_src & 7) ||
      ((uintptr_t)d_dst & 7))
    return -22;
  if (!nwords) return 0;
  hipStream_t st = (hipStream_t)stream;
#define CODESN(N) launch_codes_multi<N>(keys, d_table, capacity, d_keys, nbatches, nwords, d_src, \
                                        d_dst, d_codes, st)
  switch (keys.nkeys) {
    case 1: return CODESN(1);
    case 2: return CODESN(2);
    case 3: return CODESN(3);
    default: return CODESN(4);
  }
#undef CODESN
}

extern "C" int strom_group_agg(int type, uint32_t ops, const uint64_t *d_bitmap, uint64_t nwords,
                               const strom_filter_batch *d_vals,
                               const strom_filter_batch *d_codes, uint32_t nbatches,
                               uint64_t *d_acc, uint64_t capacity, int combine, void *stream) {
  if (!nacc_of(ops) || !nbatches || !d_bitmap || !d_vals || !d_codes || !d_acc ||
      ((uintptr_t)d_acc & 7) || !cap_ok(capacity))
    return -22;
  if (type == STROM_COL_NONE && (ops & (STROM_AGG_SUM | STROM_AGG_MIN | STROM_AGG_MAX))) return -22;
  if (!nwords) return 0;
  hipStream_t st = (hipStream_t)stream;
#define AGG(T) launch_group_agg<T>(ops, d_bitmap, nwords, d_vals, d_codes, nbatches, d_acc, \
                                   capacity + 2, combine, st)
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

// Every entry of a query over one group in one call (the host's time per
// group is on the scan's read path): entry i adds into the arrays at e[i].acc.
extern "C" int strom_group_agg_many(const strom_agg_entry *e, uint32_t n, const uint64_t *d_bitmap,
                                    uint64_t nwords, const strom_filter_batch *d_codes,
                                    uint32_t nbatches, uint64_t capacity, int combine,
                                    void *stream) {
  if (!e) return -22;
  for (uint32_t i = 0; i < n; ++i) {
    const int rc = strom_group_agg(e[i].type, e[i].ops, d_bitmap, nwords,
                                   (const strom_filter_batch *)e[i].vals, d_codes, nbatches,
                                   (uint64_t *)e[i].acc, capacity, combine, stream);
    if (rc) return rc;
  }
  return 0;
}
