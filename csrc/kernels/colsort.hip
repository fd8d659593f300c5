// colsort.hip — ORDER BY on several columns over a scan's compacted outputs
// (PG-Strom's GPU-Sort as a stage of the Arrow scan: colproject.hip leaves the
// n selected rows' values and validity bytes in HBM, this orders them).  A
// stable least-significant-digit radix sort of (key, permutation) pairs, 8
// bits a pass; the order, the buffers and the entries are specified in
// strom.h.
//
// Encode: key[i] = the order-preserving key of values[perm[i]] (coltopk.hip's
// encoding at the storage type's own width), or its class for the class pass.
//
// One pass is three launches, and no workgroup ever waits for another:
//   histogram  a workgroup owns one tile of kTile consecutive positions, counts
//              the tile's digits in LDS and stores its 256 counts into its own
//              column of the [256][ntiles] table (plain stores: deterministic);
//   scan       workgroup d turns row d of the table into exclusive prefixes,
//              a loop of kScanNT entries a trip, and stores the row's sum as
//              digit d's total behind the table (two levels: the 256 totals
//              are prefix-summed by every scatter workgroup for itself);
//   scatter    the workgroup reloads its tile; each wave owns a contiguous
//              piece and walks it 64 consecutive keys at a time.  A key's rank
//              among the equal digits of the tile is the count in earlier
//              waves, plus the wave's running count, plus the lanes below it
//              with the same digit (eight ballots) — that order makes the pass
//              stable.  The tile is staged in LDS by digit, so that a digit's
//              run leaves as consecutive addresses.
//
// Apply: out[i] = in[perm[first + i]] for the row ids and every fixed-width
// item at once; strings take their permuted lengths there, a prefix sum, and
// a character copy in output order (lanes take consecutive output dwords and
// find their row in the output offsets).
//
// The per-element work is host-device functions; strom_sort_*_host run them
// in loops over host memory (csrc/tests/colsort_fuzz.cc).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <type_traits>
#include <vector>

#include "strom/strom.h"

#define HD __host__ __device__ inline

namespace {

constexpr uint32_t kNT = 512;                  // lanes of a histogram / scatter workgroup
constexpr uint32_t kWaves = kNT / 64;
constexpr uint32_t kSteps = 8;                 // 64-key steps of a wave's piece
constexpr uint32_t kTile = STROM_SORT_TILE;    // kNT * kSteps
constexpr uint32_t kScanNT = STROM_SORT_SCAN_THREADS;
constexpr uint32_t kRadix = 256;
constexpr uint32_t kApplyNT = 256;
constexpr uint32_t kCharsGrid = 4096;          // workgroups of the character copy at most
static_assert(kTile == kNT * kSteps, "a tile is every wave's piece");

struct ApplyArgs {
  uint32_t ncols;
  strom_sort_col c[STROM_SORT_MAX_COLS];
};

HD uint32_t digit_of(uint64_t key, uint32_t shift) { return (uint32_t)(key >> shift) & 255u; }

HD uint64_t tiles_of(uint64_t n) { return (n + kTile - 1) / kTile; }

HD uint64_t width_mask(uint32_t w) { return w >= 8 ? ~0ull : (1ull << (8 * w)) - 1; }

// class (0 a value, 1 a NaN) and key of a value at its own width, before the
// direction
template <typename T> HD void encode(T x, uint64_t &key, uint32_t &cls) {
  cls = 0;
  if constexpr (std::is_floating_point<T>::value) {
    typedef typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type U;
    constexpr U sign = (U)1 << (8 * sizeof(T) - 1);
    if (x != x) {
      cls = 1;
      key = 0;
      return;
    }
    U bits;
    __builtin_memcpy(&bits, &x, sizeof(T));
    if (x == (T)0) bits = 0;                   // -0.0 is +0.0
    key = (U)((bits & sign) ? ~bits : (bits | sign));
  } else if constexpr (std::is_signed<T>::value) {
    typedef typename std::make_unsigned<T>::type U;
    key = (U)((U)x ^ ((U)1 << (8 * sizeof(T) - 1)));
  } else {
    key = (uint64_t)x;
  }
}

// key word i of an encode call
template <typename T>
HD uint64_t encode_at(const T *values, const uint8_t *valid, uint32_t p, uint64_t n, bool desc,
                      bool cls_only) {
  if (p >= n) return 0;                        // no row: apply counts it
  uint64_t key = 0;
  uint32_t cls = 2;
  if (!valid || valid[p]) encode<T>(values[p], key, cls);
  if (cls_only) return cls;
  if (cls) return 0;
  return desc ? ~key & width_mask(sizeof(T)) : key;
}

HD bool width_ok(uint32_t w) { return w == 1 || w == 2 || w == 4 || w == 8 || w == 16; }

HD void copy_fixed(uint32_t w, const uint8_t *in, uint8_t *out, uint64_t p, uint64_t i, bool ok) {
  switch (w) {
    case 1: out[i] = ok ? in[p] : 0; break;
    case 2: ((uint16_t *)out)[i] = ok ? ((const uint16_t *)in)[p] : 0; break;
    case 4: ((uint32_t *)out)[i] = ok ? ((const uint32_t *)in)[p] : 0; break;
    case 8: ((uint64_t *)out)[i] = ok ? ((const uint64_t *)in)[p] : 0; break;
    default:
      ((uint64_t *)out)[2 * i] = ok ? ((const uint64_t *)in)[2 * p] : 0;
      ((uint64_t *)out)[2 * i + 1] = ok ? ((const uint64_t *)in)[2 * p + 1] : 0;
      break;
  }
}

// output row i of an apply call; returns whether its permutation entry is a row
HD bool apply_row(const uint32_t *perm, uint64_t n, uint64_t first, uint64_t i,
                  const int64_t *rows_in, int64_t *rows_out, const strom_sort_col *c,
                  uint32_t ncols) {
  const uint64_t p = perm[first + i];
  const bool ok = p < n;
  if (rows_out) rows_out[i] = ok ? rows_in[p] : 0;
  for (uint32_t k = 0; k < ncols; ++k) {
    if (c[k].out_valid)
      ((uint8_t *)c[k].out_valid)[i] = ok ? (c[k].in_valid ? ((const uint8_t *)c[k].in_valid)[p] : 1)
                                          : 0;
    if (c[k].kind == STROM_SORT_FIXED) {
      copy_fixed(c[k].width, (const uint8_t *)c[k].in, (uint8_t *)c[k].out, p, i, ok);
    } else {
      // a string's length from its starts (n + 1 of them); a decreasing pair is empty
      int64_t len = 0;
      if (ok) {
        const int64_t a = ((const int64_t *)c[k].in)[p], e = ((const int64_t *)c[k].in)[p + 1];
        len = e > a && a >= 0 ? e - a : 0;
      }
      ((int64_t *)c[k].out)[i] = len;
    }
  }
  return ok;
}

// the output row of output byte q: the last r < count with out_off[r] <= q
HD uint64_t row_of_byte(const int64_t *out_off, uint64_t count, uint64_t q) {
  uint64_t lo = 0, hi = count;
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) >> 1;
    if ((uint64_t)out_off[mid] <= q) lo = mid;
    else hi = mid;
  }
  return lo;
}

// output dword x of a character copy: bytes 4 x .. 4 x + 3 below the total
HD void chars_quad(const uint32_t *perm, uint64_t n, uint64_t first, uint64_t count,
                   const int64_t *in_off, const uint8_t *in_chars, uint64_t in_len,
                   const int64_t *out_off, uint8_t *out_chars, uint64_t total, uint64_t x) {
  const uint64_t q0 = 4 * x;
  uint64_t r = row_of_byte(out_off, count, q0);
  uint8_t b[4] = {0, 0, 0, 0};
  uint32_t have = 0;
  for (; have < 4 && q0 + have < total; ++have) {
    const uint64_t q = q0 + have;
    while (r + 1 < count && (uint64_t)out_off[r + 1] <= q) ++r;
    const uint64_t p = perm[first + r];
    if (p >= n) continue;
    const uint64_t at = (uint64_t)in_off[p] + (q - (uint64_t)out_off[r]);
    // within the row's own characters, and within the buffer
    if (at < in_len && (int64_t)at < in_off[p + 1]) b[have] = in_chars[at];
  }
  if (have == 4 && !((uintptr_t)out_chars & 3)) {
    uint32_t w;
    __builtin_memcpy(&w, b, 4);
    ((uint32_t *)out_chars)[x] = w;
  } else {
    for (uint32_t k = 0; k < have; ++k) out_chars[q0 + k] = b[k];
  }
}

// ------------------------------------------------------------------ device
template <typename T>
__global__ __launch_bounds__(256) void sort_encode_kernel(const T *__restrict__ values,
                                                          const uint8_t *__restrict__ valid,
                                                          uint32_t *perm, uint64_t n, uint32_t flags,
                                                          uint64_t *__restrict__ key) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint32_t p = (uint32_t)i;
  if (flags & STROM_SORT_FIRST) perm[i] = p;
  else p = perm[i];
  key[i] = encode_at<T>(values, valid, p, n, (flags & STROM_SORT_DESC) != 0,
                        (flags & STROM_SORT_CLASS) != 0);
}

__global__ __launch_bounds__(kNT) void sort_hist_kernel(const uint64_t *__restrict__ key, uint64_t n,
                                                        uint32_t shift, uint32_t ntiles,
                                                        uint32_t *__restrict__ table) {
  __shared__ uint32_t h[kRadix];
  const uint32_t t = threadIdx.x;
  if (t < kRadix) h[t] = 0;
  __syncthreads();
  const uint64_t base = (uint64_t)blockIdx.x * kTile;
#pragma unroll
  for (uint32_t s = 0; s < kSteps; ++s) {
    const uint64_t i = base + s * kNT + t;
    if (i < n) atomicAdd(&h[digit_of(key[i], shift)], 1u);
  }
  __syncthreads();
  if (t < kRadix) table[(uint64_t)t * ntiles + blockIdx.x] = h[t];
}

// exclusive prefix of v over the workgroup's NW waves (red: NW words of LDS,
// free on entry; one barrier inside); total: the workgroup's sum
template <uint32_t NW>
__device__ __forceinline__ uint32_t block_exscan(uint32_t v, uint32_t *red, uint32_t &total) {
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  uint32_t inc = v;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(inc, o, 64);
    if ((int)lane >= o) inc += up;
  }
  if (lane == 63) red[wid] = inc;
  __syncthreads();
  uint32_t before = 0, all = 0;
  for (uint32_t k = 0; k < NW; ++k) {
    const uint32_t x = red[k];
    if (k < wid) before += x;
    all += x;
  }
  total = all;
  return before + inc - v;
}

__global__ __launch_bounds__(kScanNT) void sort_scan_kernel(uint32_t *__restrict__ table,
                                                            uint32_t ntiles) {
  __shared__ uint32_t red[kScanNT / 64];
  uint32_t *row = table + (uint64_t)blockIdx.x * ntiles;
  uint32_t carry = 0;
  for (uint32_t i0 = 0; i0 < ntiles; i0 += kScanNT) {
    const uint32_t i = i0 + threadIdx.x;
    const uint32_t v = i < ntiles ? row[i] : 0;
    uint32_t total;
    const uint32_t ex = block_exscan<kScanNT / 64>(v, red, total);
    if (i < ntiles) row[i] = carry + ex;
    carry += total;
    __syncthreads();                           // red is free again
  }
  if (threadIdx.x == 0) table[(uint64_t)kRadix * ntiles + blockIdx.x] = carry;
}

__global__ __launch_bounds__(kNT) void sort_scatter_kernel(
    const uint64_t *__restrict__ key_in, const uint32_t *__restrict__ perm_in,
    uint64_t *__restrict__ key_out, uint32_t *__restrict__ perm_out, uint64_t n, uint32_t shift,
    uint32_t ntiles, const uint32_t *__restrict__ table) {
  __shared__ uint64_t skey[kTile];
  __shared__ uint32_t sperm[kTile];
  __shared__ uint32_t wcnt[kWaves][kRadix];    // per wave and digit: count, then the waves before
  __shared__ uint32_t toff[kRadix];            // where a digit's run starts in the staged tile
  __shared__ uint32_t gdst[kRadix];            // ... and in the output, less toff
  __shared__ uint32_t red[kWaves];
  const uint32_t t = threadIdx.x, lane = t & 63, wid = t >> 6;
  const uint64_t base = (uint64_t)blockIdx.x * kTile;
  const uint32_t tn = (uint32_t)(n - base < kTile ? n - base : kTile);
  for (uint32_t i = t; i < kWaves * kRadix; i += kNT) (&wcnt[0][0])[i] = 0;
  __syncthreads();

  uint64_t k[kSteps];
  uint32_t p[kSteps], r[kSteps];
  const uint64_t below_me = (1ull << lane) - 1;
#pragma unroll
  for (uint32_t s = 0; s < kSteps; ++s) {
    const uint32_t j = wid * (kSteps * 64) + s * 64 + lane;
    const bool ok = j < tn;
    k[s] = ok ? key_in[base + j] : 0;
    p[s] = ok ? perm_in[base + j] : 0;
    const uint32_t d = digit_of(k[s], shift);
    uint64_t same = __ballot(ok);
#pragma unroll
    for (uint32_t b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1;
      const uint64_t bal = __ballot(bit);
      same &= bit ? bal : ~bal;
    }
    const uint32_t below = __popcll(same & below_me), all = __popcll(same);
    const uint32_t prev = wcnt[wid][d];        // every lane of the digit reads it ...
    __builtin_amdgcn_wave_barrier();
    r[s] = prev + below;
    if (ok && below + 1 == all) wcnt[wid][d] = prev + all;   // ... before its last lane adds
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();

  uint32_t mine = 0;
  if (t < kRadix) {
    for (uint32_t w = 0; w < kWaves; ++w) {
      const uint32_t c = wcnt[w][t];
      wcnt[w][t] = mine;
      mine += c;
    }
  }
  uint32_t total;
  const uint32_t ex = block_exscan<kWaves>(mine, red, total);
  __syncthreads();
  // the digits' totals behind the table: every workgroup sums the ones before
  const uint32_t dt = t < kRadix ? table[(uint64_t)kRadix * ntiles + t] : 0;
  const uint32_t dex = block_exscan<kWaves>(dt, red, total);
  if (t < kRadix) {
    toff[t] = ex;
    gdst[t] = dex + table[(uint64_t)t * ntiles + blockIdx.x] - ex;
  }
  __syncthreads();

#pragma unroll
  for (uint32_t s = 0; s < kSteps; ++s) {
    const uint32_t j = wid * (kSteps * 64) + s * 64 + lane;
    if (j < tn) {
      const uint32_t d = digit_of(k[s], shift);
      const uint32_t pos = toff[d] + wcnt[wid][d] + r[s];
      if (pos < kTile) {
        skey[pos] = k[s];
        sperm[pos] = p[s];
      }
    }
  }
  __syncthreads();
  for (uint32_t j = t; j < tn; j += kNT) {
    const uint64_t kk = skey[j];
    const uint64_t o = (uint32_t)(gdst[digit_of(kk, shift)] + j);
    if (o < n) {                               // the table is this key array's: always
      key_out[o] = kk;
      perm_out[o] = sperm[j];
    }
  }
}

__global__ __launch_bounds__(kApplyNT) void sort_apply_kernel(const uint32_t *__restrict__ perm,
                                                              uint64_t n, uint64_t first,
                                                              uint64_t count,
                                                              const int64_t *__restrict__ rows_in,
                                                              int64_t *__restrict__ rows_out,
                                                              ApplyArgs a, unsigned long long *err) {
  const uint64_t i = (uint64_t)blockIdx.x * kApplyNT + threadIdx.x;
  if (i >= count) return;
  if (!apply_row(perm, n, first, i, rows_in, rows_out, a.c, a.ncols)) atomicAdd(err, 1ull);
}

__global__ __launch_bounds__(256) void sort_chars_kernel(const uint32_t *__restrict__ perm,
                                                         uint64_t n, uint64_t first, uint64_t count,
                                                         const int64_t *__restrict__ in_off,
                                                         const uint8_t *__restrict__ in_chars,
                                                         uint64_t in_len,
                                                         const int64_t *__restrict__ out_off,
                                                         uint8_t *__restrict__ out_chars,
                                                         uint64_t out_cap) {
  uint64_t total = (uint64_t)out_off[count];
  if (total > out_cap) total = out_cap;
  const uint64_t quads = (total + 3) / 4;
  for (uint64_t x = (uint64_t)blockIdx.x * 256 + threadIdx.x; x < quads;
       x += (uint64_t)gridDim.x * 256)
    chars_quad(perm, n, first, count, in_off, in_chars, in_len, out_off, out_chars, total, x);
}

bool type_ok(int type) {
  switch (type) {
    case STROM_COL_I8: case STROM_COL_I16: case STROM_COL_I32: case STROM_COL_I64:
    case STROM_COL_U8: case STROM_COL_U16: case STROM_COL_U32: case STROM_COL_U64:
    case STROM_COL_F32: case STROM_COL_F64: return true;
    default: return false;
  }
}

constexpr uint32_t kFlags = STROM_SORT_DESC | STROM_SORT_CLASS | STROM_SORT_FIRST;

bool encode_args_ok(int type, uint32_t flags, const void *values, const void *perm, uint64_t n,
                    const void *key) {
  return type_ok(type) && !(flags & ~kFlags) && values && perm && key && !((uintptr_t)key & 7) &&
         !((uintptr_t)perm & 3) && n < (1ull << 32);
}

bool pass_args_ok(const void *ki, const void *pi, const void *ko, const void *po, uint64_t n,
                  uint32_t shift, const void *work) {
  return ki && pi && ko && po && work && ki != ko && pi != po && n < (1ull << 32) &&
         shift <= 56 && !(shift & 7) && !(((uintptr_t)ki | (uintptr_t)ko) & 7) &&
         !(((uintptr_t)pi | (uintptr_t)po | (uintptr_t)work) & 3);
}

bool apply_args_ok(const void *perm, uint64_t n, const void *rows_in, const void *rows_out,
                   const strom_sort_col *cols, uint32_t ncols, const void *err) {
  if (!perm || !err || n >= (1ull << 32) || ncols > STROM_SORT_MAX_COLS) return false;
  if (!rows_in != !rows_out || (ncols && !cols)) return false;
  for (uint32_t k = 0; k < ncols; ++k) {
    if (cols[k].kind != STROM_SORT_FIXED && cols[k].kind != STROM_SORT_LEN) return false;
    if (cols[k].kind == STROM_SORT_FIXED && !width_ok(cols[k].width)) return false;
    if (!cols[k].in || !cols[k].out) return false;
  }
  return true;
}

bool chars_args_ok(const void *perm, uint64_t n, const void *in_off, const void *in_chars,
                   const void *out_off, const void *out_chars) {
  return perm && in_off && in_chars && out_off && out_chars && n < (1ull << 32);
}

// first + count cut to the n permutation entries there are
void window(uint64_t n, uint64_t &first, uint64_t &count) {
  if (first > n) first = n;
  if (count > n - first) count = n - first;
}

template <typename T>
int host_encode(const void *values, const uint8_t *valid, uint32_t *perm, uint64_t n,
                uint32_t flags, uint64_t *key) {
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t p = (uint32_t)i;
    if (flags & STROM_SORT_FIRST) perm[i] = p;
    else p = perm[i];
    key[i] = encode_at<T>((const T *)values, valid, p, n, (flags & STROM_SORT_DESC) != 0,
                          (flags & STROM_SORT_CLASS) != 0);
  }
  return 0;
}

template <typename T>
int launch_encode(const void *values, const uint8_t *valid, uint32_t *perm, uint64_t n,
                  uint32_t flags, uint64_t *key, hipStream_t st) {
  hipLaunchKernelGGL(sort_encode_kernel<T>, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st,
                     (const T *)values, valid, perm, n, flags, key);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

}  // namespace

#define SORT_TYPES(CALL)                                  \
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

extern "C" uint64_t strom_sort_work_bytes(uint64_t n) {
  return (tiles_of(n) + 1) * kRadix * sizeof(uint32_t);
}

extern "C" int strom_sort_encode(int type, uint32_t flags, const void *d_values,
                                 const uint8_t *d_valid, uint32_t *d_perm, uint64_t n,
                                 uint64_t *d_key, void *stream) {
  if (!encode_args_ok(type, flags, d_values, d_perm, n, d_key)) return -22;
  if (!n) return 0;
#define ENCODE(T) launch_encode<T>(d_values, d_valid, d_perm, n, flags, d_key, (hipStream_t)stream)
  SORT_TYPES(ENCODE)
#undef ENCODE
}

extern "C" int strom_sort_pass(const uint64_t *d_key_in, const uint32_t *d_perm_in,
                               uint64_t *d_key_out, uint32_t *d_perm_out, uint64_t n,
                               uint32_t shift, uint32_t *d_work, void *stream) {
  if (!pass_args_ok(d_key_in, d_perm_in, d_key_out, d_perm_out, n, shift, d_work)) return -22;
  if (!n) return 0;
  hipStream_t st = (hipStream_t)stream;
  const uint32_t ntiles = (uint32_t)tiles_of(n);
  hipLaunchKernelGGL(sort_hist_kernel, dim3(ntiles), dim3(kNT), 0, st, d_key_in, n, shift, ntiles,
                     d_work);
  hipLaunchKernelGGL(sort_scan_kernel, dim3(kRadix), dim3(kScanNT), 0, st, d_work, ntiles);
  hipLaunchKernelGGL(sort_scatter_kernel, dim3(ntiles), dim3(kNT), 0, st, d_key_in, d_perm_in,
                     d_key_out, d_perm_out, n, shift, ntiles, (const uint32_t *)d_work);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int strom_sort_apply(const uint32_t *d_perm, uint64_t n, uint64_t first, uint64_t count,
                                const int64_t *d_rows_in, int64_t *d_rows_out,
                                const struct strom_sort_col *cols, uint32_t ncols, uint64_t *d_err,
                                void *stream) {
  if (!apply_args_ok(d_perm, n, d_rows_in, d_rows_out, cols, ncols, d_err)) return -22;
  window(n, first, count);
  if (!count) return 0;
  ApplyArgs a;
  memset(&a, 0, sizeof a);
  a.ncols = ncols;
  for (uint32_t k = 0; k < ncols; ++k) a.c[k] = cols[k];
  hipLaunchKernelGGL(sort_apply_kernel, dim3((uint32_t)((count + kApplyNT - 1) / kApplyNT)),
                     dim3(kApplyNT), 0, (hipStream_t)stream, d_perm, n, first, count, d_rows_in,
                     d_rows_out, a, (unsigned long long *)d_err);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

extern "C" int strom_sort_chars(const uint32_t *d_perm, uint64_t n, uint64_t first, uint64_t count,
                                const int64_t *d_in_off, const uint8_t *d_in_chars,
                                uint64_t in_len, const int64_t *d_out_off, uint8_t *d_out_chars,
                                uint64_t out_cap, void *stream) {
  if (!chars_args_ok(d_perm, n, d_in_off, d_in_chars, d_out_off, d_out_chars)) return -22;
  window(n, first, count);
  if (!count || !out_cap) return 0;
  // the characters are counted on the device: the grid is sized by the most
  // there can be, the copy's loop ends at the total
  const uint64_t most = in_len < out_cap ? in_len : out_cap;
  uint64_t grid = ((most + 3) / 4 + 255) / 256;
  grid = grid > kCharsGrid ? kCharsGrid : (grid ? grid : 1);
  hipLaunchKernelGGL(sort_chars_kernel, dim3((uint32_t)grid), dim3(256), 0, (hipStream_t)stream,
                     d_perm, n, first, count, d_in_off, d_in_chars, in_len, d_out_off, d_out_chars,
                     out_cap);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

// -------------------------------------------------------------------- host
extern "C" int strom_sort_encode_host(int type, uint32_t flags, const void *values,
                                      const uint8_t *valid, uint32_t *perm, uint64_t n,
                                      uint64_t *key) {
  if (!encode_args_ok(type, flags, values, perm, n, key)) return -22;
  if (!n) return 0;
#define ENCODE(T) host_encode<T>(values, valid, perm, n, flags, key)
  SORT_TYPES(ENCODE)
#undef ENCODE
}

extern "C" int strom_sort_pass_host(const uint64_t *key_in, const uint32_t *perm_in,
                                    uint64_t *key_out, uint32_t *perm_out, uint64_t n,
                                    uint32_t shift, uint32_t *work) {
  if (!pass_args_ok(key_in, perm_in, key_out, perm_out, n, shift, work)) return -22;
  if (!n) return 0;
  const uint64_t ntiles = tiles_of(n);
  // histogram: tile by tile into its column
  for (uint64_t tile = 0; tile < ntiles; ++tile) {
    uint32_t h[kRadix] = {0};
    const uint64_t end = (tile + 1) * kTile < n ? (tile + 1) * kTile : n;
    for (uint64_t i = tile * kTile; i < end; ++i) ++h[digit_of(key_in[i], shift)];
    for (uint32_t d = 0; d < kRadix; ++d) work[d * ntiles + tile] = h[d];
  }
  // scan: row by row, the row's sum behind the table
  for (uint32_t d = 0; d < kRadix; ++d) {
    uint32_t carry = 0;
    for (uint64_t tile = 0; tile < ntiles; ++tile) {
      const uint32_t c = work[d * ntiles + tile];
      work[d * ntiles + tile] = carry;
      carry += c;
    }
    work[kRadix * ntiles + d] = carry;
  }
  // scatter: a tile's keys in order behind their digit's run
  for (uint64_t tile = 0; tile < ntiles; ++tile) {
    uint32_t at[kRadix], dex = 0;
    for (uint32_t d = 0; d < kRadix; ++d) {
      at[d] = dex + work[d * ntiles + tile];
      dex += work[kRadix * ntiles + d];
    }
    const uint64_t end = (tile + 1) * kTile < n ? (tile + 1) * kTile : n;
    for (uint64_t i = tile * kTile; i < end; ++i) {
      const uint64_t o = at[digit_of(key_in[i], shift)]++;
      if (o < n) {
        key_out[o] = key_in[i];
        perm_out[o] = perm_in[i];
      }
    }
  }
  return 0;
}

extern "C" int strom_sort_apply_host(const uint32_t *perm, uint64_t n, uint64_t first,
                                     uint64_t count, const int64_t *rows_in, int64_t *rows_out,
                                     const struct strom_sort_col *cols, uint32_t ncols,
                                     uint64_t *err) {
  if (!apply_args_ok(perm, n, rows_in, rows_out, cols, ncols, err)) return -22;
  window(n, first, count);
  for (uint64_t i = 0; i < count; ++i)
    if (!apply_row(perm, n, first, i, rows_in, rows_out, cols, ncols)) ++*err;
  return 0;
}

extern "C" int strom_sort_chars_host(const uint32_t *perm, uint64_t n, uint64_t first,
                                     uint64_t count, const int64_t *in_off, const uint8_t *in_chars,
                                     uint64_t in_len, const int64_t *out_off, uint8_t *out_chars,
                                     uint64_t out_cap) {
  if (!chars_args_ok(perm, n, in_off, in_chars, out_off, out_chars)) return -22;
  window(n, first, count);
  if (!count || !out_cap) return 0;
  uint64_t total = (uint64_t)out_off[count];
  if (total > out_cap) total = out_cap;
  for (uint64_t x = 0; x < (total + 3) / 4; ++x)
    chars_quad(perm, n, first, count, in_off, in_chars, in_len, out_off, out_chars, total, x);
  return 0;
}
