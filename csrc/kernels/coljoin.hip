// coljoin.hip — hash join of a columnar scan's foreign-key column with a
// small dimension table (PG-Strom's pipeline is scan -> join -> pre-aggregate:
// colfilter.hip is the scan, colagg.hip the pre-aggregate, this the join).
//
// Table: open addressing with linear probing over 16-byte entries (a 64-bit
// key and a 32-bit payload, so one dwordx4 load answers a probe step), the
// capacity a power of two >= 2n.  A slot whose key is STROM_JOIN_EMPTY is
// free; that bit pattern is a legal key all the same and lives in the header
// instead.  The header (STROM_JOIN_HDR_WORDS 64-bit words in front of the
// slots) also keeps the largest displacement of any inserted key: the probe
// loop runs at most that many + 1 steps, a number the build computed — it
// never depends on the table terminating itself.
//
// Build: one thread per key, the slot claimed with a 64-bit CAS on the key
// word (global atomics execute at the memory side: only the counters see
// contention, and those are added once per wave).  The payload word is a
// plain store: the probe is a later launch.
//
// Probe: the walk of strom_column_qual and agg_flat_kernel — one wave per
// 64-row bitmap word, kU words per trip, a zero source word costs its own
// load, a row that is not selected or null issues no table load.  The home
// slots of the kU words are loaded before the first compare: beyond an XCD's
// L2 each probe is a dependent random 16-byte read, and loads in flight are
// what hides it.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "strom/strom.h"

namespace {

constexpr uint32_t kU = 4;          // words per wave and trip (as colfilter.hip)
constexpr uint32_t kMaxGrid = 8192;
constexpr uint64_t kEmpty = STROM_JOIN_EMPTY;
constexpr uint32_t kHdr = STROM_JOIN_HDR_WORDS;
typedef unsigned long long ull;

// murmur3's 64-bit finalizer
__host__ __device__ __forceinline__ uint64_t fmix64(uint64_t k) {
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

// ------------------------------------------------------------------- build
__global__ __launch_bounds__(256) void join_init_kernel(uint64_t *__restrict__ table,
                                                        uint64_t capacity) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t step = (uint64_t)gridDim.x * 256;
  if (i < kHdr) table[i] = i == STROM_JOIN_H_CAPACITY ? capacity : 0;
  for (uint64_t s = i; s < capacity; s += step) {
    table[kHdr + 2 * s] = kEmpty;
    table[kHdr + 2 * s + 1] = 0;
  }
}

__global__ __launch_bounds__(256) void join_build_kernel(const int64_t *__restrict__ keys,
                                                         const int32_t *__restrict__ payload,
                                                         uint64_t n, uint64_t *__restrict__ table,
                                                         uint64_t capacity) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t mask = capacity - 1;
  uint64_t *slots = table + kHdr;
  bool ins = false, dup = false;
  uint64_t disp = 0;
  if (i < n) {
    const uint64_t key = (uint64_t)keys[i];
    const uint32_t pay = payload ? (uint32_t)payload[i] : (uint32_t)i;
    if (key == kEmpty) {
      // the one key the slots cannot hold: a flag and its payload in the header
      if (atomicCAS((ull *)&table[STROM_JOIN_H_HAS_EMPTY], 0ull, 1ull) == 0ull) {
        table[STROM_JOIN_H_EMPTY_PAYLOAD] = pay;
        ins = true;
      } else {
        dup = true;
      }
    } else {
      uint64_t s = fmix64(key) & mask;
      // n <= capacity / 2: a free slot exists; the bound keeps the loop finite
      // whatever the arguments
      for (uint64_t d = 0; d < capacity; ++d, s = (s + 1) & mask) {
        const uint64_t old = atomicCAS((ull *)&slots[2 * s], (ull)kEmpty, (ull)key);
        if (old == kEmpty) {
          slots[2 * s + 1] = pay;
          ins = true;
          disp = d;
          break;
        }
        if (old == key) {
          dup = true;
          break;
        }
      }
    }
  }
  // the counters once per wave
  const uint32_t nins = __popcll(__ballot(ins)), ndup = __popcll(__ballot(dup));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t other = (uint64_t)__shfl_xor((ull)disp, o, 64);
    disp = other > disp ? other : disp;
  }
  if (lane == 0) {
    if (nins) atomicAdd((ull *)&table[STROM_JOIN_H_NKEYS], (ull)nins);
    if (ndup) atomicAdd((ull *)&table[STROM_JOIN_H_DUPS], (ull)ndup);
    if (disp) atomicMax((ull *)&table[STROM_JOIN_H_MAXDISP], (ull)disp);
  }
}

// ------------------------------------------------------------------- probe
// the fk of a row widened to int64; false: the value matches nothing
template <typename T> __device__ __forceinline__ bool widen(T x, uint64_t &key) {
  if constexpr (std::is_same<T, uint64_t>::value) {
    key = x;
    return x <= (uint64_t)INT64_MAX;            // compared by value
  } else {
    key = (uint64_t)(int64_t)x;
    return true;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void join_probe_kernel(const uint64_t *__restrict__ table,
                                                         uint64_t capacity,
                                                         const strom_filter_batch *__restrict__ ft,
                                                         uint32_t nb, uint64_t nwords,
                                                         const uint64_t *src, uint64_t *dst,
                                                         int anti,
                                                         const strom_filter_batch *__restrict__ kt,
                                                         ull *__restrict__ count) {
  __shared__ uint32_t wave_cnt[4];
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint64_t mask = capacity - 1;
  const ulonglong2 *slots = (const ulonglong2 *)(table + kHdr);
  // the probe loop's bound, and the key the slots cannot hold
  uint64_t maxd = table[STROM_JOIN_H_MAXDISP];
  if (maxd > mask) maxd = mask;
  const bool has_empty = table[STROM_JOIN_H_HAS_EMPTY] != 0;
  const uint32_t empty_pay = (uint32_t)table[STROM_JOIN_H_EMPTY_PAYLOAD];
  uint32_t local = 0;
  const uint64_t step = (uint64_t)gridDim.x * 4 * kU;
  for (uint64_t w0 = ((uint64_t)blockIdx.x * 4 + wid) * kU; w0 < nwords; w0 += step) {
    uint64_t raw[kU], sel[kU], key[kU], at[kU], bk[kU];
    uint32_t bi[kU];
    bool act[kU];                   // this lane probes the slots
    bool hit[kU];
    uint32_t pay[kU];
    ulonglong2 e[kU];
    // pass 1: the source word, the fk value, the home slot's load
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
      hit[u] = false;
      pay[u] = 0;
      e[u] = make_ulonglong2(kEmpty, 0);
      if (w >= nwords) continue;
      const uint64_t word = src[w];                    // uniform load, one per wave
      if (!word) continue;
      raw[u] = word;
      bi[u] = batch_of(ft, nb, w);
      const strom_filter_batch &b = ft[bi[u]];
      bk[u] = w - b.word_base;
      sel[u] = word & row_mask(b, bk[u]);
      uint64_t use = sel[u];
      if (b.valid && use) use &= ((const uint64_t *)b.valid)[bk[u]];
      if (!((use >> lane) & 1)) continue;
      if (!widen<T>(((const T *)b.values)[bk[u] * 64 + lane], key[u])) continue;
      if (key[u] == kEmpty) {
        hit[u] = has_empty;
        pay[u] = empty_pay;
        continue;
      }
      act[u] = true;
      at[u] = fmix64(key[u]) & mask;
      e[u] = slots[at[u]];
    }
    // pass 2: compare, and walk on while the slot holds another key
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u) {
      const uint64_t w = w0 + u;
      if (w >= nwords) break;
      if (sel[u]) {
        bool go = act[u];
        for (uint64_t d = 0;; ++d) {
          if (go) {
            if (e[u].x == key[u]) {
              hit[u] = true;
              pay[u] = (uint32_t)e[u].y;
              go = false;
            } else if (e[u].x == kEmpty || d >= maxd) {
              go = false;
            }
          }
          if (!__ballot(go)) break;
          if (go) {
            at[u] = (at[u] + 1) & mask;
            e[u] = slots[at[u]];
          }
        }
      }
      const uint64_t match = __ballot(hit[u]);
      const uint64_t word = anti ? sel[u] & ~match : sel[u] & match;
      if (kt && hit[u] && !anti)
        ((int32_t *)kt[bi[u]].values)[bk[u] * 64 + lane] = (int32_t)pay[u];
      // in place, a word that stays as it is (a zero one above all) is not stored
      if (lane == 0 && (dst != src || word != raw[u])) dst[w] = word;
      local += __popcll(word);
    }
  }
  if (lane == 0) wave_cnt[wid] = local;
  __syncthreads();
  if (threadIdx.x == 0 && count)
    atomicAdd(count, (ull)(wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3]));
}

template <typename T>
int launch_probe(const uint64_t *table, uint64_t capacity, const strom_filter_batch *ft,
                 uint32_t nb, uint64_t nwords, const uint64_t *src, uint64_t *dst, int anti,
                 const strom_filter_batch *kt, uint64_t *count, hipStream_t st) {
  const uint64_t g = (nwords + 4 * kU - 1) / (4 * kU);
  const uint32_t grid = (uint32_t)(g > kMaxGrid ? kMaxGrid : (g ? g : 1));
  hipLaunchKernelGGL(join_probe_kernel<T>, dim3(grid), dim3(256), 0, st, table, capacity, ft, nb,
                     nwords, src, dst, anti, kt, (ull *)count);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

// ------------------------------------------------------------- star probe
// Several dimension tables in one walk of the bitmap (a star join): leg after
// leg narrows the word, a row a leg has dropped issues no load for the legs
// behind it, and each semi leg's payload waits in a register until the last
// leg has decided the word.  The legs are a template parameter (every loop
// over them unrolls, their constants stay scalar); the storage type of a
// leg's fk column is a run-time switch around the one load.
__device__ __forceinline__ bool load_fk(uint32_t type, const void *p, uint64_t i, uint64_t &key) {
  switch (type) {
    case STROM_COL_I8: key = (uint64_t)(int64_t)((const int8_t *)p)[i]; return true;
    case STROM_COL_I16: key = (uint64_t)(int64_t)((const int16_t *)p)[i]; return true;
    case STROM_COL_I32: key = (uint64_t)(int64_t)((const int32_t *)p)[i]; return true;
    case STROM_COL_U8: key = ((const uint8_t *)p)[i]; return true;
    case STROM_COL_U16: key = ((const uint16_t *)p)[i]; return true;
    case STROM_COL_U32: key = ((const uint32_t *)p)[i]; return true;
    case STROM_COL_I64: key = ((const uint64_t *)p)[i]; return true;
    default: key = ((const uint64_t *)p)[i]; return key <= (uint64_t)INT64_MAX;   // U64
  }
}

template <int NL>
__global__ __launch_bounds__(256) void join_star_kernel(strom_join_legs legs,
                                                        const strom_filter_batch *__restrict__ ft,
                                                        uint32_t nb, uint64_t nwords,
                                                        const uint64_t *src, uint64_t *dst,
                                                        const strom_filter_batch *__restrict__ kt,
                                                        ull *__restrict__ count) {
  __shared__ uint32_t wave_cnt[4];
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  uint32_t local = 0;
  const uint64_t step = (uint64_t)gridDim.x * 4 * kU;
  for (uint64_t w0 = ((uint64_t)blockIdx.x * 4 + wid) * kU; w0 < nwords; w0 += step) {
    uint64_t raw[kU], cur[kU], bk[kU];   // the source word, the rows still in, the batch's word
    uint32_t bi[kU];
    uint32_t pay[NL][kU];
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u) {
      const uint64_t w = w0 + u;
      raw[u] = 0;
      cur[u] = 0;
      bk[u] = 0;
      bi[u] = 0;
      if (w >= nwords) continue;
      const uint64_t word = src[w];                    // uniform load, one per wave
      if (!word) continue;
      raw[u] = word;
      bi[u] = batch_of(ft, nb, w);                     // every leg's table has the same batches
      const strom_filter_batch &b = ft[bi[u]];
      bk[u] = w - b.word_base;
      cur[u] = word & row_mask(b, bk[u]);
    }
#pragma unroll
    for (int l = 0; l < NL; ++l) {
      const strom_join_leg lg = legs.leg[l];
      const uint64_t mask = lg.capacity - 1;
      const ulonglong2 *slots = (const ulonglong2 *)(lg.table + kHdr);
      uint64_t maxd = lg.table[STROM_JOIN_H_MAXDISP];
      if (maxd > mask) maxd = mask;
      uint64_t key[kU], at[kU];
      bool act[kU], hit[kU];
      ulonglong2 e[kU];
      // pass 1: the fk of the rows still in, the home slot's load
#pragma unroll
      for (uint32_t u = 0; u < kU; ++u) {
        key[u] = 0;
        at[u] = 0;
        act[u] = false;
        hit[u] = false;
        pay[l][u] = 0;
        e[u] = make_ulonglong2(kEmpty, 0);
        if (!cur[u]) continue;
        const strom_filter_batch &b = ft[(uint64_t)l * nb + bi[u]];
        uint64_t use = cur[u];
        if (b.valid) use &= ((const uint64_t *)b.valid)[bk[u]];
        if (!((use >> lane) & 1)) continue;
        if (!load_fk(lg.type, (const void *)b.values, bk[u] * 64 + lane, key[u])) continue;
        if (key[u] == kEmpty) {
          hit[u] = lg.table[STROM_JOIN_H_HAS_EMPTY] != 0;
          pay[l][u] = (uint32_t)lg.table[STROM_JOIN_H_EMPTY_PAYLOAD];
          continue;
        }
        act[u] = true;
        at[u] = fmix64(key[u]) & mask;
        e[u] = slots[at[u]];
      }
      // pass 2: compare, and walk on while the slot holds another key
#pragma unroll
      for (uint32_t u = 0; u < kU; ++u) {
        if (!cur[u]) continue;
        bool go = act[u];
        for (uint64_t d = 0;; ++d) {
          if (go) {
            if (e[u].x == key[u]) {
              hit[u] = true;
              pay[l][u] = (uint32_t)e[u].y;
              go = false;
            } else if (e[u].x == kEmpty || d >= maxd) {
              go = false;
            }
          }
          if (!__ballot(go)) break;
          if (go) {
            at[u] = (at[u] + 1) & mask;
            e[u] = slots[at[u]];
          }
        }
        const uint64_t match = __ballot(hit[u]);
        cur[u] = lg.how == STROM_JOIN_ANTI ? cur[u] & ~match : cur[u] & match;
      }
    }
    // the word is decided: the payloads of its rows, the word, the count
#pragma unroll
    for (uint32_t u = 0; u < kU; ++u) {
      const uint64_t w = w0 + u;
      if (w >= nwords) break;
      if ((cur[u] >> lane) & 1) {
#pragma unroll
        for (int l = 0; l < NL; ++l) {
          const int32_t ko = legs.leg[l].kout;
          if (ko >= 0)
            ((int32_t *)kt[(uint64_t)ko * nb + bi[u]].values)[bk[u] * 64 + lane] =
                (int32_t)pay[l][u];
        }
      }
      // in place, a word that stays as it is (a zero one above all) is not stored
      if (lane == 0 && (dst != src || cur[u] != raw[u])) dst[w] = cur[u];
      local += __popcll(cur[u]);
    }
  }
  if (lane == 0) wave_cnt[wid] = local;
  __syncthreads();
  if (threadIdx.x == 0 && count)
    atomicAdd(count, (ull)(wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3]));
}

template <int NL>
int launch_star(const strom_join_legs &legs, const strom_filter_batch *ft, uint32_t nb,
                uint64_t nwords, const uint64_t *src, uint64_t *dst, const strom_filter_batch *kt,
                uint64_t *count, hipStream_t st) {
  const uint64_t g = (nwords + 4 * kU - 1) / (4 * kU);
  const uint32_t grid = (uint32_t)(g > kMaxGrid ? kMaxGrid : (g ? g : 1));
  hipLaunchKernelGGL(join_star_kernel<NL>, dim3(grid), dim3(256), 0, st, legs, ft, nb, nwords, src,
                     dst, kt, (ull *)count);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

bool pow2(uint64_t x) { return x && !(x & (x - 1)); }

bool fk_type(uint32_t t) {
  switch (t) {
    case STROM_COL_I8: case STROM_COL_I16: case STROM_COL_I32: case STROM_COL_I64:
    case STROM_COL_U8: case STROM_COL_U16: case STROM_COL_U32: case STROM_COL_U64:
      return true;
    default:
      return false;       // floats, strings, bool, decimal: no integer key
  }
}

}  // namespace

extern "C" uint64_t strom_join_capacity(uint64_t n) {
  uint64_t c = 64;
  while (c < 2 * n) c <<= 1;
  return c;
}

extern "C" uint64_t strom_join_hash(int64_t key) { return fmix64((uint64_t)key); }

extern "C" int strom_join_build(const int64_t *d_keys, const int32_t *d_payload, uint64_t n,
                                uint64_t *d_table, uint64_t capacity, void *stream) {
  if (!d_table || ((uintptr_t)d_table & 15) || (n && !d_keys)) return -22;
  if (!pow2(capacity) || capacity < 64 || capacity < 2 * n || capacity > (1ull << 40)) return -22;
  hipStream_t st = (hipStream_t)stream;
  uint64_t g = (capacity + 255) / 256;
  hipLaunchKernelGGL(join_init_kernel, dim3((uint32_t)(g > kMaxGrid ? kMaxGrid : g)), dim3(256), 0,
                     st, d_table, capacity);
  if (hipGetLastError() != hipSuccess) return -5;
  if (!n) return 0;
  g = (n + 255) / 256;
  if (g > 0x7fffffffull) return -22;
  hipLaunchKernelGGL(join_build_kernel, dim3((uint32_t)g), dim3(256), 0, st, d_keys, d_payload, n,
                     d_table, capacity);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int strom_column_join(int type, int how, const uint64_t *d_table, uint64_t capacity,
                                 const strom_filter_batch *d_fk, uint32_t nbatches,
                                 uint64_t nwords, const uint64_t *d_src, uint64_t *d_dst,
                                 const strom_filter_batch *d_kout, uint64_t *d_count,
                                 void *stream) {
  if (!d_table || ((uintptr_t)d_table & 15) || !pow2(capacity) || capacity < 64) return -22;
  if (!d_fk || !nbatches || !d_src || !d_dst || ((uintptr_t)d_src & 7) || ((uintptr_t)d_dst & 7))
    return -22;
  if (how != STROM_JOIN_SEMI && how != STROM_JOIN_ANTI) return -22;
  if (d_kout && how == STROM_JOIN_ANTI) return -22;   // a row that stays matched nothing
  if (!nwords) return 0;
  hipStream_t st = (hipStream_t)stream;
#define JOIN(T) launch_probe<T>(d_table, capacity, d_fk, nbatches, nwords, d_src, d_dst, \
                                how == STROM_JOIN_ANTI, d_kout, d_count, st)
  switch (type) {
    case STROM_COL_I8: return JOIN(int8_t);
    case STROM_COL_I16: return JOIN(int16_t);
    case STROM_COL_I32: return JOIN(int32_t);
    case STROM_COL_I64: return JOIN(int64_t);
    case STROM_COL_U8: return JOIN(uint8_t);
    case STROM_COL_U16: return JOIN(uint16_t);
    case STROM_COL_U32: return JOIN(uint32_t);
    case STROM_COL_U64: return JOIN(uint64_t);
    default: return -22;        // floats, strings, bool, decimal: no integer key
  }
#undef JOIN
}

extern "C" int strom_column_join_star(struct strom_join_legs legs,
                                      const strom_filter_batch *d_fk, uint32_t nbatches,
                                      uint64_t nwords, const uint64_t *d_src, uint64_t *d_dst,
                                      const strom_filter_batch *d_kout, uint64_t *d_count,
                                      void *stream) {
  if (!legs.nlegs || legs.nlegs > STROM_JOIN_MAX_LEGS) return -22;
  uint32_t outs = 0;                                  // the code tables taken so far
  for (uint32_t l = 0; l < legs.nlegs; ++l) {
    const strom_join_leg &g = legs.leg[l];
    if (!g.table || ((uintptr_t)g.table & 15) || !pow2(g.capacity) || g.capacity < 64) return -22;
    if (!fk_type(g.type)) return -22;
    if (g.how != STROM_JOIN_SEMI && g.how != STROM_JOIN_ANTI) return -22;
    if (g.kout < -1 || g.kout >= STROM_JOIN_MAX_LEGS) return -22;
    if (g.kout >= 0) {
      if (g.how == STROM_JOIN_ANTI || !d_kout) return -22;   // a row that stays matched nothing
      if (outs & (1u << g.kout)) return -22;                 // one leg per code table
      outs |= 1u << g.kout;
    }
  }
  if (!d_fk || !nbatches || !d_src || !d_dst || ((uintptr_t)d_src & 7) || ((uintptr_t)d_dst & 7))
    return -22;
  if (!nwords) return 0;
  hipStream_t st = (hipStream_t)stream;
  switch (legs.nlegs) {
    case 1: return launch_star<1>(legs, d_fk, nbatches, nwords, d_src, d_dst, d_kout, d_count, st);
    case 2: return launch_star<2>(legs, d_fk, nbatches, nwords, d_src, d_dst, d_kout, d_count, st);
    case 3: return launch_star<3>(legs, d_fk, nbatches, nwords, d_src, d_dst, d_kout, d_count, st);
    default: return launch_star<4>(legs, d_fk, nbatches, nwords, d_src, d_dst, d_kout, d_count, st);
  }
}
