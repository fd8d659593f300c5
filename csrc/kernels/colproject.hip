// colproject.hip — a select list: the selected rows' ids and up to
// STROM_PROJ_MAX_COLS projected columns in one walk of the selection bitmap
// (strom_bitmap_to_rows_multi; Arrow scans: scan_where(quals, project=[...])).
//
// colfilter.hip's single-column emit has each lane walk its own bitmap word
// and store to its own output run (neighbouring lanes 8 * popcount bytes
// apart) and copies characters one byte per lane-iteration.  Here the
// rank -> row map of a 256-word block is built once, in LDS and in output
// order, as 16-bit local row numbers (256 words = 16,384 rows), and every
// column is a loop over output positions with the lane as the fast index:
// the row ids and every fixed-width column are stored coalesced, the loads
// are the gather.  Characters are copied in output order too: a string
// column goes through the block's rows in chunks, the starts of a chunk's
// rows are prefix-summed in LDS, and the lanes take consecutive dwords of
// the chunk's output bytes and find their row in that prefix.
//
// Three launches whatever the select list: per-block counts (rows, and per
// string column characters), one scan launch that offsets each count array
// by its device cursor and advances the cursor, and the emit.
//
// Bits at or past a batch's rows are ignored (counted and emitted by
// neither launch), so no set of bitmap words makes a column's buffers be
// read outside the rows their batch table declares.
//
// strom_bitmap_to_rows_multi_host is the same walk in plain C++: the
// kernel's reference (tests/test_gpu_arrow_project.py) and the target of
// csrc/tests/colproject_fuzz.cc.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <map>
#include <mutex>
#include <type_traits>
#include <utility>

#include "strom/strom.h"

namespace {

constexpr uint32_t kWordsPerBlock = 256;
constexpr uint32_t kBlockRows = kWordsPerBlock * 64;   // local row numbers fit 16 bits
constexpr uint32_t kChunk = 512;                        // rows of a string column per LDS prefix
constexpr uint32_t kChunkPer = kChunk / 256;            // ... per thread

// the select list as a kernel argument (the caller's descriptors are host
// memory: nothing to upload, nothing to keep alive)
struct ProjArgs {
  uint32_t ncols;
  uint32_t nstr;                                  // string columns: count arrays 1..nstr
  strom_proj_col c[STROM_PROJ_MAX_COLS];
};

struct ScanArgs {
  uint64_t cursor[STROM_PROJ_MAX_COLS + 1];       // device cursor of each count array
};

__host__ __device__ inline bool is_str(int32_t kind) {
  return kind == STROM_PROJ_STR32 || kind == STROM_PROJ_STR64;
}

// batch of bitmap word w: the last b with word_base <= w
__host__ __device__ inline uint32_t batch_of(const strom_filter_batch *b, uint32_t nb, uint64_t w) {
  uint32_t lo = 0, hi = nb;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (b[mid].word_base <= w) lo = mid;
    else hi = mid;
  }
  return lo;
}

// the bits of word w that are rows of batch b (local0: the word's first row)
__host__ __device__ inline uint64_t row_bits(uint64_t word, uint64_t w, const strom_filter_batch &b,
                                             uint64_t &local0) {
  local0 = (w - b.word_base) * 64;
  if (w < b.word_base || local0 >= b.nrows) return 0;
  const uint64_t left = b.nrows - local0;
  return left >= 64 ? word : word & ((1ull << left) - 1);
}

// A selected row's characters (offsets of `wide` ? 8 : 4 bytes, the
// characters in aux): a malformed offset pair gives an empty string, never
// a read outside the buffer.
__host__ __device__ inline void str_span(const void *offs, bool wide, uint64_t aux_len, uint64_t r,
                                         uint64_t &s, uint32_t &len) {
  int64_t a, e;
  if (wide) {
    a = ((const int64_t *)offs)[r];
    e = ((const int64_t *)offs)[r + 1];
  } else {
    a = ((const int32_t *)offs)[r];
    e = ((const int32_t *)offs)[r + 1];
  }
  const bool ok = a >= 0 && e >= a && (uint64_t)e <= aux_len;
  s = ok ? (uint64_t)a : 0;
  len = ok ? (uint32_t)(e - a) : 0;
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
  for (int o = 32; o > 0; o >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, o, 64);
  return v;
}

// exclusive prefix of v over the 256 threads (red: 4 words of LDS, free on
// entry; a barrier inside); total: the block's sum
template <typename T>
__device__ __forceinline__ T block_exscan(T v, T *red, T &total) {
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  T inc = v;
  for (int o = 1; o < 64; o <<= 1) {
    const T up = (T)__shfl_up((unsigned long long)inc, o, 64);
    if ((int)lane >= o) inc += up;
  }
  if (lane == 63) red[wid] = inc;
  __syncthreads();
  T before = 0, all = 0;
  for (uint32_t k = 0; k < 4; ++k) {
    const T x = red[k];
    if (k < wid) before += x;
    all += x;
  }
  total = all;
  return before + inc - v;
}

// per 256-word block: cnt[blk] = its selected rows, cnt[(1 + j) * nblk + blk]
// = the characters of string column j's selected rows
__global__ __launch_bounds__(256) void proj_count_kernel(const uint64_t *__restrict__ bm,
                                                         uint64_t nwords,
                                                         const strom_filter_batch *__restrict__ bt,
                                                         uint32_t nb, ProjArgs pa,
                                                         uint64_t *__restrict__ cnt) {
  __shared__ uint64_t red[4];
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint64_t w = (uint64_t)blockIdx.x * kWordsPerBlock + threadIdx.x;
  uint64_t word = w < nwords ? bm[w] : 0, local0 = 0;
  uint32_t bi = 0;
  if (word) {
    bi = batch_of(bt, nb, w);
    word = row_bits(word, w, bt[bi], local0);
  }
  uint32_t j = 0;
  for (uint32_t a = 0; a <= pa.ncols; ++a) {
    // a == 0: the rows; a > 0: column a - 1 when it is a string column
    uint64_t sum = 0;
    if (a == 0) {
      sum = __popcll(word);
    } else {
      const strom_proj_col &c = pa.c[a - 1];
      if (!is_str(c.kind)) continue;
      if (word) {
        const strom_qual_batch q = ((const strom_qual_batch *)c.table)[bi];
        for (uint64_t x = word; x; x &= x - 1) {
          uint64_t st;
          uint32_t len;
          str_span((const void *)q.values, c.kind == STROM_PROJ_STR64, q.aux_len,
                   local0 + (__ffsll((unsigned long long)x) - 1), st, len);
          sum += len;
        }
      }
    }
    sum = wave_sum(sum);
    __syncthreads();                      // red is free again
    if (lane == 0) red[wid] = sum;
    __syncthreads();
    if (threadIdx.x == 0)
      cnt[(uint64_t)j * gridDim.x + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
    ++j;
  }
}

// colfilter.hip's scan_blocks_cursor_kernel for every count array in one
// launch: workgroup a turns array a into exclusive prefixes offset by its
// cursor, which it then advances (every thread reads the cursor before the
// first barrier, thread 1023 writes it after the last)
__global__ __launch_bounds__(1024) void proj_scan_kernel(uint64_t *__restrict__ cnt_all, uint32_t nb,
                                                         ScanArgs sa) {
  __shared__ uint64_t part[1024];
  uint64_t *cnt = cnt_all + (uint64_t)blockIdx.x * nb;
  unsigned long long *cursor = (unsigned long long *)sa.cursor[blockIdx.x];
  const uint32_t t = threadIdx.x;
  const uint64_t base = *cursor;
  const uint32_t per = (nb + 1023) / 1024;
  const uint32_t lo = min(nb, t * per), hi = min(nb, lo + per);
  uint64_t s = 0;
  for (uint32_t i = lo; i < hi; ++i) s += cnt[i];
  part[t] = s;
  __syncthreads();
  for (uint32_t off = 1; off < 1024; off <<= 1) {
    uint64_t add = t >= off ? part[t - off] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  uint64_t run = base + (t ? part[t - 1] : 0);
  for (uint32_t i = lo; i < hi; ++i) {
    const uint64_t c = cnt[i];
    cnt[i] = run;
    run += c;
  }
  if (t == 1023) *cursor = base + part[1023];
}

struct __attribute__((packed)) U32Unaligned { uint32_t v; };

// gather of one fixed-width column: four output positions per thread and
// trip, their loads issued before the first store
template <uint32_t W>
__device__ __forceinline__ void gather_fixed(const uint16_t *rowsel, const uint64_t *wloc,
                                             const uint64_t *vptr, uint32_t nsel, uint8_t *out) {
  typedef typename std::conditional<W == 1, uint8_t, typename std::conditional<W == 2, uint16_t,
          typename std::conditional<W == 4, uint32_t, uint64_t>::type>::type>::type T;
  constexpr uint32_t N = W == 16 ? 2 : 1;
  for (uint32_t p0 = threadIdx.x; p0 < nsel; p0 += 4 * 256) {
    T x[4][N];
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u) {
      const uint32_t p = p0 + u * 256;
      if (p < nsel) {
        const uint32_t r = rowsel[p];
        const T *src = (const T *)vptr[r >> 6] + (wloc[r >> 6] + (r & 63)) * N;
#pragma unroll
        for (uint32_t k = 0; k < N; ++k) x[u][k] = src[k];
      }
    }
#pragma unroll
    for (uint32_t u = 0; u < 4; ++u) {
      const uint32_t p = p0 + u * 256;
      if (p < nsel) {
#pragma unroll
        for (uint32_t k = 0; k < N; ++k) ((T *)out)[(uint64_t)p * N + k] = x[u][k];
      }
    }
  }
}

// STR: the kernel is instantiated without the string stage's LDS for select
// lists of fixed-width columns only
template <bool STR>
__global__ __launch_bounds__(256) void proj_emit_kernel(const uint64_t *__restrict__ bm,
                                                        uint64_t nwords,
                                                        const strom_filter_batch *__restrict__ bt,
                                                        uint32_t nb, ProjArgs pa,
                                                        const uint64_t *__restrict__ base,
                                                        int64_t *__restrict__ out) {
  __shared__ uint16_t rowsel[kBlockRows];       // rank -> local row, in output order
  __shared__ uint64_t wloc[256];                // per word: its first row within its batch
  __shared__ uint32_t wbi[256];                 // ... and its batch
  // per word and column: the batch's buffers (p0 first holds the words'
  // first global row ids: the row ids are written before any column)
  __shared__ uint64_t p0[256], p1[256];
  __shared__ uint64_t p2[STR ? 256 : 1], p3[STR ? 256 : 1];
  __shared__ uint64_t csrc[STR ? kChunk : 1];   // a chunk's rows: where their characters are
  __shared__ uint64_t cst[STR ? kChunk + 1 : 1];   // ... and start in the chunk's output
  __shared__ uint64_t red[4];

  const uint32_t tid = threadIdx.x;
  const uint32_t nblk = gridDim.x;
  const uint64_t w = (uint64_t)blockIdx.x * kWordsPerBlock + tid;
  uint64_t word = w < nwords ? bm[w] : 0, local0 = 0;
  uint32_t bi = 0;
  if (word) {
    bi = batch_of(bt, nb, w);
    const strom_filter_batch b = bt[bi];
    word = row_bits(word, w, b, local0);
    p0[tid] = b.row_base + local0;
  }
  wloc[tid] = local0;
  wbi[tid] = bi;
  const uint32_t c = __popcll(word);
  uint32_t nsel;
  uint32_t pos = block_exscan<uint32_t>(c, (uint32_t *)red, nsel);
  if (!nsel) return;                           // uniform: no row of the block is selected
  for (uint64_t x = word; x; x &= x - 1)
    rowsel[pos++] = (uint16_t)(tid * 64 + (__ffsll((unsigned long long)x) - 1));
  __syncthreads();

  const uint64_t rbase = base[blockIdx.x];
  for (uint32_t p = tid; p < nsel; p += 256) {
    const uint32_t r = rowsel[p];
    out[rbase + p] = (int64_t)(p0[r >> 6] + (r & 63));
  }

  uint32_t j = 0;                               // string columns before this one
  for (uint32_t ci = 0; ci < pa.ncols; ++ci) {
    const strom_proj_col &col = pa.c[ci];
    const bool str = is_str(col.kind);
    __syncthreads();                            // the previous column's pointers are done with
    if (word) {
      const strom_qual_batch *q = (const strom_qual_batch *)col.table + wbi[tid];
      p0[tid] = q->values;
      p1[tid] = q->valid;
      if (STR && str) {
        p2[tid] = q->aux;
        p3[tid] = q->aux_len;
      }
    }
    __syncthreads();
    uint8_t *ov = (uint8_t *)col.out_valid;
    if (ov && !str) {
      for (uint32_t p = tid; p < nsel; p += 256) {
        const uint32_t r = rowsel[p];
        const uint8_t *val = (const uint8_t *)p1[r >> 6];
        const uint64_t row = wloc[r >> 6] + (r & 63);
        ov[rbase + p] = val ? (val[row >> 3] >> (row & 7)) & 1 : 1;
      }
    }
    if (col.kind == STROM_PROJ_FIXED) {
      uint8_t *o = (uint8_t *)col.out + rbase * col.width;
      switch (col.width) {
        case 1: gather_fixed<1>(rowsel, wloc, p0, nsel, o); break;
        case 2: gather_fixed<2>(rowsel, wloc, p0, nsel, o); break;
        case 4: gather_fixed<4>(rowsel, wloc, p0, nsel, o); break;
        case 8: gather_fixed<8>(rowsel, wloc, p0, nsel, o); break;
        default: gather_fixed<16>(rowsel, wloc, p0, nsel, o); break;
      }
    } else if (col.kind == STROM_PROJ_BOOL) {
      uint8_t *o = (uint8_t *)col.out + rbase;
      for (uint32_t p = tid; p < nsel; p += 256) {
        const uint32_t r = rowsel[p];
        const uint64_t row = wloc[r >> 6] + (r & 63);
        o[p] = (((const uint8_t *)p0[r >> 6])[row >> 3] >> (row & 7)) & 1;
      }
    } else if (STR && str) {
      const bool wide = col.kind == STROM_PROJ_STR64;
      const uint64_t cbase = base[(uint64_t)(1 + j) * nblk + blockIdx.x];
      int64_t *ostart = (int64_t *)col.out + rbase;
      uint8_t *ochars = (uint8_t *)col.out_chars;
      uint64_t cacc = 0;                        // characters of the chunks before (uniform)
      for (uint32_t c0 = 0; c0 < nsel; c0 += kChunk) {
        const uint32_t n = min(kChunk, nsel - c0);
        // each row's source and length, the lane the fast index
        for (uint32_t q = tid; q < kChunk; q += 256) {
          uint64_t st = 0;
          uint32_t len = 0;
          if (q < n) {
            const uint32_t r = rowsel[c0 + q];
            const uint32_t wi = r >> 6;
            const uint64_t row = wloc[wi] + (r & 63);
            str_span((const void *)p0[wi], wide, p3[wi], row, st, len);
            st += p2[wi];
            if (ov) {
              const uint8_t *val = (const uint8_t *)p1[wi];
              ov[rbase + c0 + q] = val ? (val[row >> 3] >> (row & 7)) & 1 : 1;
            }
          }
          csrc[q] = st;
          cst[q] = len;
        }
        __syncthreads();
        // lengths -> starts: each thread its kChunkPer consecutive rows
        uint64_t l[kChunkPer], sum = 0, total;
#pragma unroll
        for (uint32_t k = 0; k < kChunkPer; ++k) {
          l[k] = cst[tid * kChunkPer + k];
          sum += l[k];
        }
        uint64_t ex = block_exscan<uint64_t>(sum, red, total);
#pragma unroll
        for (uint32_t k = 0; k < kChunkPer; ++k) {
          cst[tid * kChunkPer + k] = ex;
          ex += l[k];
        }
        if (tid == 255) cst[kChunk] = total;
        __syncthreads();
        const uint64_t d0 = cbase + cacc;       // the chunk's first output byte
        for (uint32_t q = tid; q < n; q += 256) ostart[c0 + q] = (int64_t)(d0 + cst[q]);
        // the chunk's bytes: lane u takes the aligned dword u of the output,
        // of which bytes [lo, hi) belong to the chunk
        const uint64_t addr0 = (uint64_t)(uintptr_t)ochars + d0;
        const uint32_t skew = (uint32_t)(addr0 & 3);
        const uint64_t nunits = (skew + total + 3) / 4;
        for (uint64_t u = tid; u < nunits; u += 256) {
          const int64_t at = (int64_t)(4 * u) - skew;        // chunk-relative first byte
          const uint64_t first = at < 0 ? 0 : (uint64_t)at;
          const uint64_t end = (uint64_t)(at + 4) < total ? (uint64_t)(at + 4) : total;
          // the row of `first`: the last q with cst[q] <= first
          uint32_t lo = 0, hi = n;
          while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (cst[mid] <= first) lo = mid;
            else hi = mid;
          }
          uint8_t *dst = ochars + d0 + at;
          const uint64_t rend = lo + 1 < n ? cst[lo + 1] : total;
          if (at >= 0 && end == (uint64_t)at + 4 && end <= rend) {
            // a whole dword from one row
            const uint32_t v = ((const U32Unaligned *)((const uint8_t *)csrc[lo] + (first - cst[lo])))->v;
            *(uint32_t *)dst = v;
          } else {
            uint32_t v = 0;
            for (uint64_t b = first; b < end; ++b) {
              while (lo + 1 < n && cst[lo + 1] <= b) ++lo;
              v |= (uint32_t)((const uint8_t *)csrc[lo])[b - cst[lo]] << (8 * (uint32_t)(b - at));
            }
            if (at >= 0 && end == (uint64_t)at + 4) {
              *(uint32_t *)dst = v;
            } else {
              // the chunk's first or last dword: only its own bytes are stored
              for (uint64_t b = first; b < end; ++b) dst[b - at] = (uint8_t)(v >> (8 * (uint32_t)(b - at)));
            }
          }
        }
        cacc += total;
        __syncthreads();                        // csrc / cst are free again
      }
      ++j;
    }
  }
}

// Block-count scratch of the launches, kept per (device, stream) and grown
// on demand, as colfilter.hip keeps its own (stream-ordered reuse on one
// stream is safe; hipMallocAsync blocked the host behind the stream's work)
struct Scratch {
  void *p = nullptr;
  size_t bytes = 0;
  uint64_t used = 0;
};
std::mutex g_mu;
std::map<std::pair<int, void *>, Scratch> g_scratch;
uint64_t g_clock = 0;
constexpr size_t kKeep = 64;

// under g_mu, held by the caller through its launches
void *scratch(hipStream_t st, size_t bytes) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  const std::pair<int, void *> key{dev, (void *)st};
  if (!g_scratch.count(key) && g_scratch.size() >= kKeep) {
    auto lru = g_scratch.begin();
    for (auto j = g_scratch.begin(); j != g_scratch.end(); ++j)
      if (j->second.used < lru->second.used) lru = j;
    if (lru->second.p) (void)hipFree(lru->second.p);
    g_scratch.erase(lru);
  }
  Scratch &e = g_scratch[key];
  e.used = ++g_clock;
  if (e.bytes < bytes) {
    // the old buffer may still be read by this stream's queued launches
    if (e.p && (hipStreamSynchronize(st) != hipSuccess || hipFree(e.p) != hipSuccess))
      return nullptr;
    e.p = nullptr;
    e.bytes = 0;
    const size_t want = bytes < (64u << 10) ? (64u << 10) : bytes;
    void *p = nullptr;
    if (hipMalloc(&p, want) != hipSuccess) return nullptr;
    e.p = p;
    e.bytes = want;
  }
  return e.p;
}

// the checks both entry points share; nstr: the string columns
int check_cols(const strom_proj_col *cols, uint32_t ncols, uint32_t *nstr) {
  if (!cols || !ncols || ncols > STROM_PROJ_MAX_COLS) return -22;
  *nstr = 0;
  for (uint32_t i = 0; i < ncols; ++i) {
    const strom_proj_col &c = cols[i];
    if (!c.table || !c.out) return -22;
    switch (c.kind) {
      case STROM_PROJ_FIXED:
        if (c.width != 1 && c.width != 2 && c.width != 4 && c.width != 8 && c.width != 16)
          return -22;
        if (c.out & ((c.width == 16 ? 8 : c.width) - 1)) return -22;
        break;
      case STROM_PROJ_BOOL:
        break;
      case STROM_PROJ_STR32:
      case STROM_PROJ_STR64:
        if (!c.out_chars || !c.char_cursor || (c.out & 7) || (c.char_cursor & 7)) return -22;
        // a cursor shared by two columns would be advanced twice
        for (uint32_t k = 0; k < i; ++k)
          if (is_str(cols[k].kind) && cols[k].char_cursor == c.char_cursor) return -22;
        ++*nstr;
        break;
      default:
        return -22;
    }
  }
  return 0;
}

void host_store(uint64_t out, uint64_t pos, const void *src, uint32_t width) {
  std::memcpy((uint8_t *)out + pos * width, src, width);
}

}  // namespace

extern "C" int strom_bitmap_to_rows_multi(const uint64_t *d_bitmap, uint64_t nwords,
                                          const strom_filter_batch *d_batches, uint32_t nbatches,
                                          int64_t *d_out, uint64_t *d_total,
                                          const strom_proj_col *cols, uint32_t ncols,
                                          void *stream) {
  if (!nwords || !nbatches) return 0;
  if (!d_bitmap || !d_batches || !d_out || !d_total || ((uintptr_t)d_bitmap & 7) ||
      ((uintptr_t)d_out & 7) || ((uintptr_t)d_total & 7))
    return -22;
  ProjArgs pa{};
  if (int rc = check_cols(cols, ncols, &pa.nstr)) return rc;
  pa.ncols = ncols;
  ScanArgs sa{};
  sa.cursor[0] = (uint64_t)(uintptr_t)d_total;
  for (uint32_t i = 0, j = 0; i < ncols; ++i) {
    pa.c[i] = cols[i];
    if (is_str(cols[i].kind)) sa.cursor[++j] = cols[i].char_cursor;
  }
  hipStream_t st = (hipStream_t)stream;
  const uint64_t nb64 = (nwords + kWordsPerBlock - 1) / kWordsPerBlock;
  if (nb64 > 0xffffffffull) return -75;
  const uint32_t nb = (uint32_t)nb64;
  std::lock_guard<std::mutex> g(g_mu);
  uint64_t *cnt = (uint64_t *)scratch(st, sizeof(uint64_t) * (1 + pa.nstr) * nb);
  if (!cnt) return -12;
  hipLaunchKernelGGL(proj_count_kernel, dim3(nb), dim3(256), 0, st, d_bitmap, nwords, d_batches,
                     nbatches, pa, cnt);
  hipLaunchKernelGGL(proj_scan_kernel, dim3(1 + pa.nstr), dim3(1024), 0, st, cnt, nb, sa);
  if (pa.nstr)
    hipLaunchKernelGGL(proj_emit_kernel<true>, dim3(nb), dim3(256), 0, st, d_bitmap, nwords,
                       d_batches, nbatches, pa, cnt, d_out);
  else
    hipLaunchKernelGGL(proj_emit_kernel<false>, dim3(nb), dim3(256), 0, st, d_bitmap, nwords,
                       d_batches, nbatches, pa, cnt, d_out);
  return hipGetLastError() == hipSuccess ? 0 : -5;
}

// The host copy: one pass over the words, every pointer host memory
// (unaligned buffers are fine: every access is a memcpy).
extern "C" int strom_bitmap_to_rows_multi_host(const uint64_t *bitmap, uint64_t nwords,
                                               const strom_filter_batch *batches,
                                               uint32_t nbatches, int64_t *out, uint64_t *total,
                                               const strom_proj_col *cols, uint32_t ncols) {
  if (!nwords || !nbatches) return 0;
  if (!bitmap || !batches || !out || !total || ((uintptr_t)bitmap & 7) || ((uintptr_t)out & 7) ||
      ((uintptr_t)total & 7))
    return -22;
  uint32_t nstr = 0;
  if (int rc = check_cols(cols, ncols, &nstr)) return rc;
  if ((nwords + kWordsPerBlock - 1) / kWordsPerBlock > 0xffffffffull) return -75;
  uint64_t pos = *total;
  for (uint64_t w = 0; w < nwords; ++w) {
    if (!bitmap[w]) continue;
    const uint32_t bi = batch_of(batches, nbatches, w);
    const strom_filter_batch &b = batches[bi];
    uint64_t local0;
    for (uint64_t x = row_bits(bitmap[w], w, b, local0); x; x &= x - 1, ++pos) {
      const uint64_t r = local0 + (uint64_t)__builtin_ctzll(x);
      out[pos] = (int64_t)(b.row_base + r);
      for (uint32_t i = 0; i < ncols; ++i) {
        const strom_proj_col &c = cols[i];
        strom_qual_batch q;
        std::memcpy(&q, (const uint8_t *)c.table + sizeof(q) * bi, sizeof(q));
        if (c.out_valid) {
          const uint8_t *val = (const uint8_t *)q.valid;
          ((uint8_t *)c.out_valid)[pos] = val ? (val[r >> 3] >> (r & 7)) & 1 : 1;
        }
        if (c.kind == STROM_PROJ_FIXED) {
          host_store(c.out, pos, (const uint8_t *)q.values + r * c.width, c.width);
        } else if (c.kind == STROM_PROJ_BOOL) {
          ((uint8_t *)c.out)[pos] = (((const uint8_t *)q.values)[r >> 3] >> (r & 7)) & 1;
        } else {
          const bool wide = c.kind == STROM_PROJ_STR64;
          const uint32_t ow = wide ? 8 : 4;
          // the offset pair through a copy: the file's buffer may be unaligned
          alignas(8) uint8_t pair[16];
          std::memcpy(pair, (const uint8_t *)q.values + r * ow, 2 * ow);
          uint64_t s;
          uint32_t len;
          str_span(pair, wide, q.aux_len, 0, s, len);
          uint64_t *cur = (uint64_t *)c.char_cursor;
          const int64_t start = (int64_t)*cur;
          host_store(c.out, pos, &start, 8);
          if (len) std::memcpy((uint8_t *)c.out_chars + *cur, (const uint8_t *)q.aux + s, len);
          *cur += len;
        }
      }
    }
  }
  *total = pos;
  return 0;
}
