// coltopk.hip — ORDER BY one column LIMIT k over a columnar scan's selection
// bitmap (PG-Strom's GPU-Sort + LIMIT as a stage of the Arrow scan's group
// pipeline: colfilter.hip / coljoin.hip leave the bitmap, this keeps the k
// best rows of it).  The order, the candidate words, the state and the slabs
// are specified in strom.h.
//
// Select: the walk of join_probe_kernel — one wave per 64-row bitmap word, a
// zero word costs its own load.  A workgroup takes four words per trip; the
// rows that pass the state's threshold key (read once, one 64-bit load) and
// the workgroup's own k-th candidate so far are appended to a buffer in LDS at
// a cursor the wave adds to once.  Between two trips the fill is looked at:
// past the limit the buffer is sorted (bitonic, in LDS), cut to k and its k-th
// candidate becomes the workgroup's threshold.  The last sort leaves the slab.
//
// Merge: one workgroup, the same buffer: the state's candidates, then every
// slab's that still beat the k-th (a slab is sorted: the first that does not
// ends it), sorted and cut the same way.
//
// Every phase is a host-device function of (buffer, thread): the kernels run
// them over the lanes with barriers between, strom_topk_host_* over a loop.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>
#include <vector>

#include "strom/strom.h"

#define HD __host__ __device__ inline

namespace {

constexpr uint32_t kNT = 256;          // lanes of a workgroup: four words per trip
constexpr uint32_t kMinWords = 16;     // words a workgroup walks at least
constexpr uint32_t kMaxGrid = 1024;
constexpr uint32_t kSlabEntries = 1u << 18;   // grid * k stays below
constexpr uint64_t kSign = 1ull << 63;
constexpr uint32_t kHdr = STROM_TOPK_HDR_WORDS;
constexpr uint32_t kSlabHdr = STROM_TOPK_SLAB_HDR_WORDS;
constexpr uint32_t kEnt = STROM_TOPK_ENTRY_WORDS;
constexpr uint64_t kPass = ~0ull;      // the threshold that passes everything
typedef unsigned long long ull;

struct Ent {
  uint64_t key, meta, pay;
};

// the candidate buffer: three arrays of cap words (LDS, or the host's heap)
struct Buf {
  uint64_t *key, *meta, *pay;
  HD Ent get(uint32_t i) const { return Ent{key[i], meta[i], pay[i]}; }
  HD void put(uint32_t i, const Ent &e) const {
    key[i] = e.key;
    meta[i] = e.meta;
    pay[i] = e.pay;
  }
};

HD bool ent_less(const Ent &a, const Ent &b) {
  const uint64_t ca = a.meta >> 62, cb = b.meta >> 62;
  if (ca != cb) return ca < cb;
  if (a.key != b.key) return a.key < b.key;
  return a.meta < b.meta;
}

// behind every candidate (class 3 is never a row's)
HD Ent ent_last() { return Ent{~0ull, ~0ull, ~0ull}; }

HD uint32_t pow2_ceil(uint32_t n) {
  uint32_t p = 1;
  while (p < n) p <<= 1;
  return p;
}

// entries of the buffer for k: the fill past which it is compacted — twice k,
// so that a sort pays for k appends at least — and a trip's appends
constexpr uint32_t kMaxEntries = STROM_TOPK_MAX_K + kNT;
HD uint32_t buf_entries(uint32_t k) {
  const uint32_t c = (2 * k > 64 ? 2 * k : 64) + kNT;
  return c > kMaxEntries ? kMaxEntries : c;
}
HD uint32_t buf_limit(uint32_t cap) { return cap - kNT; }

// one compare-exchange of the bitonic network over the power of two >= n:
// pair t of the stage (kk, j), j == kk / 2 its first.  The network is the
// normalized one — a stage's first step pairs i with its mirror in the block
// of kk, the others with i + j, and every exchange puts the smaller first — so
// the entries at and beyond n, which would all be "behind every candidate",
// never move and need no storage: a pair that reaches there is skipped.
HD void bitonic_step(const Buf &b, uint32_t n, uint32_t kk, uint32_t j, uint32_t t) {
  uint32_t i, l;
  if (j == kk >> 1) {
    i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
    l = (i | (kk - 1)) - (t & (j - 1));
  } else {
    i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
    l = i + j;
  }
  if (l >= n) return;
  const Ent x = b.get(i), y = b.get(l);
  if (ent_less(y, x)) {
    b.put(i, y);
    b.put(l, x);
  }
}

HD uint32_t batch_of(const strom_filter_batch *b, uint32_t nb, uint64_t w) {
  uint32_t lo = 0, hi = nb;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (b[mid].word_base <= w) lo = mid;
    else hi = mid;
  }
  return lo;
}

// rows of batch word k that exist
HD uint64_t row_mask(const strom_filter_batch &b, uint64_t k) {
  if (k * 64 >= b.nrows) return 0;
  const uint64_t rem = b.nrows - k * 64;
  return rem >= 64 ? ~0ull : (1ull << rem) - 1;
}

// class, key and the -0.0 flag of a value (the key before the direction)
template <typename T> HD void encode(T x, uint64_t &key, uint64_t &cls, uint64_t &negz) {
  cls = 0;
  negz = 0;
  if constexpr (std::is_floating_point<T>::value) {
    const double d = (double)x;
    if (d != d) {
      cls = 1;
      key = 0;
      return;
    }
    uint64_t bits;
    __builtin_memcpy(&bits, &d, 8);
    if (d == 0.0) {
      negz = bits >> 63;
      bits = 0;
    }
    key = (bits & kSign) ? ~bits : (bits | kSign);
  } else if constexpr (std::is_signed<T>::value) {
    key = (uint64_t)(int64_t)x ^ kSign;
  } else {
    key = (uint64_t)x;
  }
}

HD uint64_t load_pay(uint64_t base, uint32_t width, uint64_t row) {
  switch (width) {
    case 1: return ((const uint8_t *)base)[row];
    case 2: return ((const uint16_t *)base)[row];
    case 4: return ((const uint32_t *)base)[row];
    default: return ((const uint64_t *)base)[row];
  }
}

// the candidate of lane's row of batch word bk
template <typename T>
HD Ent make_entry(const strom_filter_batch &vb, const strom_filter_batch *pb, uint32_t pw,
                  uint64_t bk, uint32_t lane, bool desc) {
  const uint64_t row = bk * 64 + lane;
  uint64_t key = 0, cls = 2, negz = 0, pv = 0, pay = 0;
  if (!vb.valid || ((((const uint64_t *)vb.valid)[bk] >> lane) & 1)) {
    encode<T>(((const T *)vb.values)[row], key, cls, negz);
    if (desc && cls == 0) key = ~key;
  }
  if (pb && (!pb->valid || ((((const uint64_t *)pb->valid)[bk] >> lane) & 1))) {
    pv = 1;
    pay = load_pay(pb->values, pw, row);
  }
  return Ent{key, cls << 62 | (vb.row_base + row) << 2 | negz << 1 | pv, pay};
}

HD bool passes(const Ent &e, uint64_t thresh) {
  return thresh == kPass || ((e.meta >> 62) == 0 && e.key <= thresh);
}

HD uint64_t thresh_of(const Ent &kth) { return (kth.meta >> 62) == 0 ? kth.key : kPass; }

// ------------------------------------------------------------------ device
// the workgroup's buffer state besides the entries
struct Wg {
  uint32_t count;       // entries held
  uint32_t has_thr;     // thr is the k-th candidate of a compaction
  Ent thr;
};

// sort, cut to k, tighten: every lane calls it between two barriers' worth of
// quiet (no lane appends while another is in here)
__device__ void wg_compact(const Buf &b, Wg *wg, uint32_t k, uint32_t cap) {
  const uint32_t t = threadIdx.x;
  const uint32_t n = wg->count > cap ? cap : wg->count;
  const uint32_t p = pow2_ceil(n > 2 ? n : 2);
  __syncthreads();                       // every lane has read the fill
  for (uint32_t kk = 2; kk <= p; kk <<= 1)
    for (uint32_t j = kk >> 1; j > 0; j >>= 1) {
      for (uint32_t i = t; i < p / 2; i += kNT) bitonic_step(b, n, kk, j, i);
      __syncthreads();
    }
  if (t == 0) {
    wg->count = n < k ? n : k;
    if (n >= k) {
      wg->has_thr = 1;
      wg->thr = b.get(k - 1);
    }
  }
  __syncthreads();
}

// the fill as every lane sees it between two trips
__device__ __forceinline__ uint32_t wg_fill(const Wg *wg) {
  __syncthreads();
  const uint32_t n = wg->count;
  __syncthreads();                       // ... before any lane appends again
  return n;
}

__device__ __forceinline__ void wave_append(const Buf &b, Wg *wg, uint32_t cap, bool cand,
                                            const Ent &e, uint32_t lane) {
  const uint64_t bal = __ballot(cand);
  if (!bal) return;
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(&wg->count, (uint32_t)__popcll(bal));
  base = __shfl(base, 0, 64);
  if (cand) {
    const uint32_t pos = base + __popcll(bal & ((1ull << lane) - 1));
    if (pos < cap) b.put(pos, e);        // the limit keeps it below
  }
}

template <typename T>
__global__ __launch_bounds__(kNT) void topk_select_kernel(
    uint32_t k, uint32_t cap, int desc, const uint64_t *__restrict__ bitmap, uint64_t nwords,
    const strom_filter_batch *__restrict__ vt, const strom_filter_batch *__restrict__ pt,
    uint32_t pw, uint32_t nb, const uint64_t *state, uint64_t *__restrict__ slabs) {
  extern __shared__ __attribute__((aligned(16))) uint64_t topk_lds[];   // key, meta, pay
  __shared__ Wg wg;
  __shared__ uint32_t seen_of[4];
  const Buf b{topk_lds, topk_lds + cap, topk_lds + 2 * (uint64_t)cap};
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint32_t limit = buf_limit(cap);
  if (threadIdx.x == 0) {
    wg.count = 0;
    wg.has_thr = 0;
  }
  // the one look at the state: a merge on another stream may store a smaller
  // key meanwhile, and this one then passes rows the result does not need
  const uint64_t thresh = __atomic_load_n(&state[STROM_TOPK_H_THRESH], __ATOMIC_RELAXED);
  uint32_t seen = 0;
  for (uint64_t w0 = (uint64_t)blockIdx.x * 4; w0 < nwords; w0 += (uint64_t)gridDim.x * 4) {
    if (wg_fill(&wg) > limit) wg_compact(b, &wg, k, cap);
    const uint64_t w = w0 + wid;
    if (w >= nwords) continue;
    const uint64_t word = bitmap[w];                   // uniform load, one per wave
    if (!word) continue;
    const strom_filter_batch &vb = vt[batch_of(vt, nb, w)];
    const uint64_t bk = w - vb.word_base;
    const uint64_t sel = word & row_mask(vb, bk);
    if (!sel) continue;
    seen += __popcll(sel);
    bool cand = false;
    Ent e = ent_last();
    if ((sel >> lane) & 1) {
      e = make_entry<T>(vb, pt ? &pt[&vb - vt] : nullptr, pw, bk, lane, desc != 0);
      cand = passes(e, thresh) && !(wg.has_thr && !ent_less(e, wg.thr));
    }
    wave_append(b, &wg, cap, cand, e, lane);
  }
  wg_fill(&wg);
  wg_compact(b, &wg, k, cap);
  if (lane == 0) seen_of[wid] = seen;
  __syncthreads();
  uint64_t *slab = slabs + (uint64_t)blockIdx.x * (kSlabHdr + (uint64_t)kEnt * k);
  const uint32_t n = wg.count;
  if (threadIdx.x == 0) {
    slab[0] = n;
    slab[1] = (uint64_t)seen_of[0] + seen_of[1] + seen_of[2] + seen_of[3];
  }
  for (uint32_t i = threadIdx.x; i < n; i += kNT) {
    const Ent x = b.get(i);
    slab[kSlabHdr + kEnt * i] = x.key;
    slab[kSlabHdr + kEnt * i + 1] = x.meta;
    slab[kSlabHdr + kEnt * i + 2] = x.pay;
  }
}

__global__ __launch_bounds__(kNT) void topk_init_kernel(uint64_t *state, uint32_t k) {
  if (threadIdx.x < kHdr)
    state[threadIdx.x] = threadIdx.x == STROM_TOPK_H_K ? k
                         : threadIdx.x == STROM_TOPK_H_THRESH ? kPass : 0;
}

__global__ __launch_bounds__(kNT) void topk_merge_kernel(uint32_t k, uint32_t cap,
                                                         const uint64_t *__restrict__ slabs,
                                                         uint32_t nslabs, uint64_t *state) {
  extern __shared__ __attribute__((aligned(16))) uint64_t topk_lds[];
  __shared__ Wg wg;
  const Buf b{topk_lds, topk_lds + cap, topk_lds + 2 * (uint64_t)cap};
  const uint32_t t = threadIdx.x;
  const uint32_t limit = buf_limit(cap);
  const uint64_t n0 = state[STROM_TOPK_H_COUNT];
  if (state[STROM_TOPK_H_K] != k || n0 > k) {          // not a state of this k
    __syncthreads();
    if (t == 0) state[STROM_TOPK_H_ERRORS] += 1;
    return;
  }
  for (uint32_t i = t; i < n0; i += kNT)
    b.put(i, Ent{state[kHdr + kEnt * i], state[kHdr + kEnt * i + 1], state[kHdr + kEnt * i + 2]});
  if (t == 0) {
    wg.count = (uint32_t)n0;
    wg.has_thr = 0;
  }
  __syncthreads();
  if (t == 0 && n0 == k) {
    wg.has_thr = 1;
    wg.thr = b.get(k - 1);
  }
  uint64_t seen = 0, errors = 0;
  const uint64_t sw = kSlabHdr + (uint64_t)kEnt * k;
  for (uint32_t s = 0; s < nslabs; ++s) {
    const uint64_t *slab = slabs + s * sw;
    const uint64_t n = slab[0];
    if (n > k) {                                       // refused whole
      ++errors;
      continue;
    }
    seen += slab[1];
    for (uint32_t i0 = 0; i0 < n; i0 += kNT) {
      if (wg_fill(&wg) > limit) wg_compact(b, &wg, k, cap);
      const uint64_t *at = slab + kSlabHdr + (uint64_t)kEnt * i0;
      // sorted: behind one that no longer beats the k-th nothing does
      if (wg.has_thr && !ent_less(Ent{at[0], at[1], at[2]}, wg.thr)) break;
      const uint32_t i = i0 + t;
      bool cand = false;
      Ent e = ent_last();
      if (i < n) {
        at = slab + kSlabHdr + (uint64_t)kEnt * i;
        e = Ent{at[0], at[1], at[2]};
        cand = (e.meta >> 62) < 3 && !(wg.has_thr && !ent_less(e, wg.thr));
      }
      wave_append(b, &wg, cap, cand, e, t & 63);
    }
  }
  wg_fill(&wg);
  wg_compact(b, &wg, k, cap);
  const uint32_t n = wg.count;
  for (uint32_t i = t; i < n; i += kNT) {
    const Ent x = b.get(i);
    state[kHdr + kEnt * i] = x.key;
    state[kHdr + kEnt * i + 1] = x.meta;
    state[kHdr + kEnt * i + 2] = x.pay;
  }
  if (t == 0) {
    state[STROM_TOPK_H_COUNT] = n;
    state[STROM_TOPK_H_SEEN] += seen;
    state[STROM_TOPK_H_ERRORS] += errors;
    state[STROM_TOPK_H_MERGES] += 1;
    if (n == k) state[STROM_TOPK_H_THRESH] = thresh_of(b.get(k - 1));
  }
}

// more LDS than the 64 KiB a kernel gets unasked (up to the CU's 160 KiB)
template <typename K> bool allow_lds(K kernel, uint32_t bytes) {
  if (bytes <= (64u << 10)) return true;
  return hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)bytes) == hipSuccess;
}

template <typename T>
int launch_select(uint32_t k, int desc, const uint64_t *bitmap, uint64_t nwords,
                  const strom_filter_batch *vt, const strom_filter_batch *pt, uint32_t pw,
                  uint32_t nb, const uint64_t *state, uint64_t *slabs, hipStream_t st) {
  const uint32_t cap = buf_entries(k), lds = cap * kEnt * 8;
  if (!allow_lds(topk_select_kernel<T>, lds)) return -5;
  hipLaunchKernelGGL(topk_select_kernel<T>, dim3(strom_column_topk_grid(nwords, k)), dim3(kNT),
                     lds, st, k, cap, desc, bitmap, nwords, vt, pt, pw, nb, state, slabs);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

// -------------------------------------------------------------------- host
// the same phases, a workgroup's lanes one after the other
struct HostBuf {
  std::vector<uint64_t> words;
  Buf b;
  uint32_t cap, limit, k, count = 0;
  bool has_thr = false;
  Ent thr{};
  explicit HostBuf(uint32_t k_) : words((size_t)buf_entries(k_) * kEnt), cap(buf_entries(k_)),
                                  limit(buf_limit(buf_entries(k_))), k(k_) {
    b = Buf{words.data(), words.data() + cap, words.data() + 2 * (size_t)cap};
  }
  void compact() {
    const uint32_t n = count > cap ? cap : count;
    const uint32_t p = pow2_ceil(n > 2 ? n : 2);
    for (uint32_t kk = 2; kk <= p; kk <<= 1)
      for (uint32_t j = kk >> 1; j > 0; j >>= 1)
        for (uint32_t i = 0; i < p / 2; ++i) bitonic_step(b, n, kk, j, i);
    count = n < k ? n : k;
    if (n >= k) {
      has_thr = true;
      thr = b.get(k - 1);
    }
  }
  void append(const Ent &e) {
    if (count < cap) b.put(count, e);
    ++count;
  }
  bool beats(const Ent &e) const { return !(has_thr && !ent_less(e, thr)); }
};

template <typename T>
int host_select(uint32_t k, bool desc, const uint64_t *bitmap, uint64_t nwords,
                const strom_filter_batch *vt, const strom_filter_batch *pt, uint32_t pw,
                uint32_t nb, const uint64_t *state, uint64_t *slabs) {
  const uint32_t grid = strom_column_topk_grid(nwords, k);
  const uint64_t thresh = state[STROM_TOPK_H_THRESH];
  for (uint32_t g = 0; g < grid; ++g) {
    HostBuf h(k);
    uint64_t seen = 0;
    for (uint64_t w0 = (uint64_t)g * 4; w0 < nwords; w0 += (uint64_t)grid * 4) {
      if (h.count > h.limit) h.compact();
      // the lanes of a trip compare with the threshold the trip began with
      const bool has_thr = h.has_thr;
      const Ent thr = h.thr;
      for (uint32_t wid = 0; wid < 4; ++wid) {
        const uint64_t w = w0 + wid;
        if (w >= nwords) continue;
        const uint64_t word = bitmap[w];
        if (!word) continue;
        const strom_filter_batch &vb = vt[batch_of(vt, nb, w)];
        const uint64_t bk = w - vb.word_base;
        const uint64_t sel = word & row_mask(vb, bk);
        seen += (uint64_t)__builtin_popcountll(sel);
        for (uint32_t lane = 0; lane < 64; ++lane) {
          if (!((sel >> lane) & 1)) continue;
          const Ent e = make_entry<T>(vb, pt ? &pt[&vb - vt] : nullptr, pw, bk, lane, desc);
          if (passes(e, thresh) && !(has_thr && !ent_less(e, thr))) h.append(e);
        }
      }
    }
    h.compact();
    uint64_t *slab = slabs + (uint64_t)g * (kSlabHdr + (uint64_t)kEnt * k);
    slab[0] = h.count;
    slab[1] = seen;
    for (uint32_t i = 0; i < h.count; ++i) {
      const Ent x = h.b.get(i);
      slab[kSlabHdr + kEnt * i] = x.key;
      slab[kSlabHdr + kEnt * i + 1] = x.meta;
      slab[kSlabHdr + kEnt * i + 2] = x.pay;
    }
  }
  return 0;
}

bool type_ok(int type) {
  switch (type) {
    case STROM_COL_I8: case STROM_COL_I16: case STROM_COL_I32: case STROM_COL_I64:
    case STROM_COL_U8: case STROM_COL_U16: case STROM_COL_U32: case STROM_COL_U64:
    case STROM_COL_F32: case STROM_COL_F64: return true;
    default: return false;
  }
}

bool select_args_ok(int type, uint32_t flags, uint32_t k, const void *bitmap, const void *vals,
                    const void *pay, uint32_t pw, uint32_t nb, const void *state,
                    const void *slabs) {
  if (!type_ok(type) || (flags & ~(uint32_t)STROM_TOPK_DESC)) return false;
  if (k < 1 || k > STROM_TOPK_MAX_K) return false;
  if (!bitmap || ((uintptr_t)bitmap & 7) || !vals || !nb || !state || ((uintptr_t)state & 7) ||
      !slabs || ((uintptr_t)slabs & 7))
    return false;
  if (pay ? (pw != 1 && pw != 2 && pw != 4 && pw != 8) : pw != 0) return false;
  return true;
}

}  // namespace

extern "C" uint64_t strom_topk_state_words(uint32_t k) { return kHdr + (uint64_t)kEnt * k; }

extern "C" uint64_t strom_topk_slab_words(uint32_t k) { return kSlabHdr + (uint64_t)kEnt * k; }

extern "C" uint32_t strom_column_topk_grid(uint64_t nwords, uint32_t k) {
  if (!nwords || !k) return 0;
  uint32_t most = kSlabEntries / k;
  most = most > kMaxGrid ? kMaxGrid : (most ? most : 1);
  const uint64_t g = (nwords + kMinWords - 1) / kMinWords;
  return (uint32_t)(g > most ? most : g);
}

#define TOPK_TYPES(CALL)                                  \
  switch (type) {                                         \
    case STROM_COL_I8: return CALL(int8_t);               \
    case STROM_COL_I16: return CALL(int16_t);             \
    case STROM_COL_I32: return CALL(int32_t);             \
    case STROM_COL_I64: return CALL(int64_t);             \
    case STROM_COL_U8: return CALL(uint8_t);              \
    case STROM_COL_U16: return CALL(uint16_t);            \
    case STROM_COL_U32: return CALL(uint32_t);            \
    case STROM_COL_U64: return CALL(uint64_t);            \
    case STROM_COL_F32: return CALL(float);               \
    case STROM_COL_F64: return CALL(double);              \
    default: return -22;                                  \
  }

extern "C" int strom_topk_init(uint64_t *d_state, uint32_t k, void *stream) {
  if (!d_state || ((uintptr_t)d_state & 7) || k < 1 || k > STROM_TOPK_MAX_K) return -22;
  hipLaunchKernelGGL(topk_init_kernel, dim3(1), dim3(kNT), 0, (hipStream_t)stream, d_state, k);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int strom_column_topk(int type, uint32_t flags, uint32_t k, const uint64_t *d_bitmap,
                                 uint64_t nwords, const strom_filter_batch *d_vals,
                                 const strom_filter_batch *d_pay, uint32_t pay_width,
                                 uint32_t nbatches, const uint64_t *d_state, uint64_t *d_slabs,
                                 void *stream) {
  if (!select_args_ok(type, flags, k, d_bitmap, d_vals, d_pay, pay_width, nbatches, d_state,
                      d_slabs))
    return -22;
  if (!nwords) return 0;
  hipStream_t st = (hipStream_t)stream;
#define SELECT(T) launch_select<T>(k, (int)(flags & STROM_TOPK_DESC), d_bitmap, nwords, d_vals, \
                                   d_pay, pay_width, nbatches, d_state, d_slabs, st)
  TOPK_TYPES(SELECT)
#undef SELECT
}

extern "C" int strom_topk_merge(uint32_t k, const uint64_t *d_slabs, uint32_t nslabs,
                                uint64_t *d_state, void *stream) {
  if (!d_state || ((uintptr_t)d_state & 7) || k < 1 || k > STROM_TOPK_MAX_K) return -22;
  if (nslabs && (!d_slabs || ((uintptr_t)d_slabs & 7))) return -22;
  if (!nslabs) return 0;
  const uint32_t cap = buf_entries(k), lds = cap * kEnt * 8;
  if (!allow_lds(topk_merge_kernel, lds)) return -5;
  hipLaunchKernelGGL(topk_merge_kernel, dim3(1), dim3(kNT), lds, (hipStream_t)stream, k, cap,
                     d_slabs, nslabs, d_state);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int strom_topk_host_init(uint64_t *state, uint32_t k) {
  if (!state || k < 1 || k > STROM_TOPK_MAX_K) return -22;
  for (uint32_t i = 0; i < kHdr; ++i) state[i] = 0;
  state[STROM_TOPK_H_K] = k;
  state[STROM_TOPK_H_THRESH] = kPass;
  return 0;
}

extern "C" int strom_topk_host_select(int type, uint32_t flags, uint32_t k,
                                      const uint64_t *bitmap, uint64_t nwords,
                                      const strom_filter_batch *vals,
                                      const strom_filter_batch *pay, uint32_t pay_width,
                                      uint32_t nbatches, const uint64_t *state, uint64_t *slabs) {
  if (!select_args_ok(type, flags, k, bitmap, vals, pay, pay_width, nbatches, state, slabs))
    return -22;
  if (!nwords) return 0;
#define SELECT(T) host_select<T>(k, (flags & STROM_TOPK_DESC) != 0, bitmap, nwords, vals, pay, \
                                 pay_width, nbatches, state, slabs)
  TOPK_TYPES(SELECT)
#undef SELECT
}

extern "C" int strom_topk_host_merge(uint32_t k, const uint64_t *slabs, uint32_t nslabs,
                                     uint64_t *state) {
  if (!state || k < 1 || k > STROM_TOPK_MAX_K || (nslabs && !slabs)) return -22;
  if (!nslabs) return 0;
  const uint64_t n0 = state[STROM_TOPK_H_COUNT];
  if (state[STROM_TOPK_H_K] != k || n0 > k) {
    state[STROM_TOPK_H_ERRORS] += 1;
    return 0;
  }
  HostBuf h(k);
  for (uint32_t i = 0; i < n0; ++i)
    h.append(Ent{state[kHdr + kEnt * i], state[kHdr + kEnt * i + 1], state[kHdr + kEnt * i + 2]});
  if (n0 == k) {
    h.has_thr = true;
    h.thr = h.b.get(k - 1);
  }
  uint64_t seen = 0, errors = 0;
  const uint64_t sw = kSlabHdr + (uint64_t)kEnt * k;
  for (uint32_t s = 0; s < nslabs; ++s) {
    const uint64_t *slab = slabs + s * sw;
    const uint64_t n = slab[0];
    if (n > k) {
      ++errors;
      continue;
    }
    seen += slab[1];
    for (uint32_t i0 = 0; i0 < n; i0 += kNT) {
      if (h.count > h.limit) h.compact();
      const uint64_t *at = slab + kSlabHdr + (uint64_t)kEnt * i0;
      if (!h.beats(Ent{at[0], at[1], at[2]})) break;
      const bool has_thr = h.has_thr;
      const Ent thr = h.thr;
      for (uint32_t i = i0; i < n && i < i0 + kNT; ++i) {
        at = slab + kSlabHdr + (uint64_t)kEnt * i;
        const Ent e{at[0], at[1], at[2]};
        if ((e.meta >> 62) < 3 && !(has_thr && !ent_less(e, thr))) h.append(e);
      }
    }
  }
  h.compact();
  for (uint32_t i = 0; i < h.count; ++i) {
    const Ent x = h.b.get(i);
    state[kHdr + kEnt * i] = x.key;
    state[kHdr + kEnt * i + 1] = x.meta;
    state[kHdr + kEnt * i + 2] = x.pay;
  }
  state[STROM_TOPK_H_COUNT] = h.count;
  state[STROM_TOPK_H_SEEN] += seen;
  state[STROM_TOPK_H_ERRORS] += errors;
  state[STROM_TOPK_H_MERGES] += 1;
  if (h.count == k) state[STROM_TOPK_H_THRESH] = thresh_of(h.b.get(k - 1));
  return 0;
}
