// collike.hip — SQL LIKE on utf8 / binary columns (STROM_QOP_STR_LIKE of
// strom_column_qual; `contains` and `endswith` are the patterns %x% and %x).
//
// A pattern is cut at its '%' into segments (strom.h has the operand
// layout); a segment is literal pieces with runs of '_' around them.  A row
// matches when
//   - the first segment matches at the row's first byte (no leading '%'),
//   - the last one matches backwards from the row's last byte (no trailing
//     '%') and does not begin before the point the head ended at,
//   - every segment between is found, leftmost-first, from where the one
//     before it ended, before the tail.
// Leftmost-first needs no backtracking across a '%': where a segment can end
// is a non-decreasing function of where it starts (a literal advances by its
// length, a '_' to the next byte that continues no character), so the
// leftmost match leaves the longest remainder, and whatever a later match
// could be followed by, the leftmost one can be followed by too.
//
// '_' is one byte on a binary column.  On a utf8 column it is one byte and
// every 0x80-0xBF byte directly after it: one code point on valid UTF-8, and
// defined the same way on bytes that are not (file data).  Backwards it
// steps over the 0x80-0xBF bytes before the position, then one byte more.
//
// The walk is qual_kernel's (colfilter.hip): one wave per bitmap word, one
// row per lane, the batch by binary search, the operands staged in LDS.  Per
// row: the offset check, the length reject against the pattern's least
// bytes, the head, the tail, the middle segments.  Literals are compared as
// str_eq does: aligned dword loads funnel-shifted into place (v_alignbyte),
// never a dword that holds no byte of the row; a '_' on utf8 reads single
// bytes of the row.  A pattern without '_' (STROM_QUAL_LIKE_WILD clear) has
// its own instantiation: a byte search whose candidates are rejected by one
// masked dword compare of the needle's first four bytes, the row's dwords
// loaded once as the window slides.
//
// With one row per lane a wave takes as long as its longest search, so a
// row whose middle segments have more than STROM_LIKE_LONG_ROW bytes to be
// searched in (what is left of a long row once head and tail are compared:
// those cost the same on either path) is set aside by a ballot and then
// matched one row per wave: head and tail by every lane alike (a uniform
// compare), a searched segment at 64 consecutive candidate positions at a
// time, the leftmost hit by ballot + find-first.  Both paths find the
// leftmost match, so they give the same bits.
//
// Cost: every loop is bounded by the row's length, a segment's pieces or the
// pattern's segments.  The worst case is a self-overlapping needle on a
// long row of one repeated letter ('%aaaaaaab%' on 'aaaa...'): every
// candidate compares nearly the whole needle, len x segment bytes.  There
// are no skip tables (Boyer-Moore, two-way).
//
// Limit: positions in a row are 32-bit (the length is cast as colfilter.hip's
// string operators cast it) and 0xffffffff stands for "no match", so a row
// of a large_utf8 column has to be shorter than 4 GiB; a longer one is
// matched on its length modulo 2^32, still inside the row.
//
// strom_column_like_host is the same matcher compiled for the host (the
// ballots become loops over 64 lanes), for the sanitizer run of
// csrc/tests/collike_fuzz.cc.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdlib>

#include "strom/strom.h"

namespace {

#define HD __host__ __device__ inline

constexpr uint32_t kNo = 0xffffffffu;   // no match (a position otherwise)

HD uint32_t funnel(uint32_t hi, uint32_t lo, uint32_t sh) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbyte(hi, lo, sh);
#else
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * sh));
#endif
}

// len > 0 bytes at p == the constant c (4-aligned): str_eq of colfilter.hip
HD bool lit_eq(const uint8_t *p, const uint32_t *c, uint32_t len) {
  const uintptr_t a = (uintptr_t)p;
  const uint32_t *w = (const uint32_t *)(a & ~(uintptr_t)3);
  const uint32_t *last = (const uint32_t *)((a + len - 1) & ~(uintptr_t)3);
  const uint32_t sh = (uint32_t)(a & 3);
  uint32_t cur = *w;
  for (uint32_t j = 0; j < len; j += 4) {
    const uint32_t *nx = w + 1 <= last ? w + 1 : last;
    const uint32_t nxt = *nx;
    const uint32_t v = funnel(nxt, cur, sh);
    const uint32_t rem = len - j;
    const uint32_t m = rem >= 4 ? ~0u : (1u << (8 * rem)) - 1;
    if ((v ^ c[j >> 2]) & m) return false;
    cur = nxt;
    ++w;
  }
  return true;
}

HD bool is_cont(uint8_t b) { return (b & 0xC0) == 0x80; }

// k '_' forwards from p (p <= lim): the position after them, kNo past lim
template <bool UTF8>
HD uint32_t skip_fwd(const uint8_t *r, uint32_t p, uint32_t lim, uint32_t k) {
  if (!UTF8) return lim - p >= k ? p + k : kNo;
  for (; k; --k) {
    if (p >= lim) return kNo;
    ++p;
    while (p < lim && is_cont(r[p])) ++p;
  }
  return p;
}

// k '_' backwards from e (e >= lo): the position before them, kNo below lo
template <bool UTF8>
HD uint32_t skip_bwd(const uint8_t *r, uint32_t e, uint32_t lo, uint32_t k) {
  if (!UTF8) return e - lo >= k ? e - k : kNo;
  for (; k; --k) {
    if (e <= lo) return kNo;
    --e;
    while (e > lo && is_cont(r[e])) --e;
  }
  return e;
}

// the segment at p, inside [p, lim): where it ends, or kNo
template <bool WILD, bool UTF8>
HD uint32_t seg_fwd(const uint8_t *r, uint32_t p, uint32_t lim, const uint32_t *cs,
                    const uint32_t *seg) {
  const uint32_t np = seg[1];
  const uint32_t *pc = seg + 3;
  for (uint32_t i = 0; i < np; ++i, pc += 3) {
    if (WILD && pc[0]) {
      p = skip_fwd<UTF8>(r, p, lim, pc[0]);
      if (p == kNo) return kNo;
    }
    const uint32_t L = pc[2];
    if (lim - p < L || !lit_eq(r + p, cs + pc[1] / 4, L)) return kNo;
    p += L;
  }
  if (WILD && seg[2]) p = skip_fwd<UTF8>(r, p, lim, seg[2]);
  return p;
}

// the segment ending at e, inside [lo, e): where it begins, or kNo
template <bool WILD, bool UTF8>
HD uint32_t seg_bwd(const uint8_t *r, uint32_t e, uint32_t lo, const uint32_t *cs,
                    const uint32_t *seg) {
  const uint32_t np = seg[1];
  if (WILD && seg[2]) {
    e = skip_bwd<UTF8>(r, e, lo, seg[2]);
    if (e == kNo) return kNo;
  }
  const uint32_t *pc = seg + 3 + 3 * np;
  for (uint32_t i = 0; i < np; ++i) {
    pc -= 3;
    const uint32_t L = pc[2];
    if (e - lo < L || !lit_eq(r + e - L, cs + pc[1] / 4, L)) return kNo;
    e -= L;
    if (WILD && pc[0]) {
      e = skip_bwd<UTF8>(r, e, lo, pc[0]);
      if (e == kNo) return kNo;
    }
  }
  return e;
}

// leftmost occurrence of the L > 0 bytes c in [cur, end): where it ends.
// The row's dwords are loaded once as the window slides; a candidate is
// rejected by the masked compare of the needle's first dword.
HD uint32_t lit_find(const uint8_t *r, uint32_t cur, uint32_t end, const uint32_t *c, uint32_t L) {
  if (end - cur < L) return kNo;
  const uint32_t c0 = c[0];
  const uint32_t m0 = L >= 4 ? ~0u : (1u << (8 * L)) - 1;
  const uintptr_t a = (uintptr_t)(r + cur);
  const uint32_t *w = (const uint32_t *)(a & ~(uintptr_t)3);
  const uint32_t *last = (const uint32_t *)(((uintptr_t)r + end - 1) & ~(uintptr_t)3);
  uint32_t sh = (uint32_t)(a & 3);
  uint32_t lo = *w;
  uint32_t hi = *(w + 1 <= last ? w + 1 : last);
  const uint32_t stop = end - L;
  for (uint32_t p = cur; p <= stop; ++p) {
    const uint32_t v = funnel(hi, lo, sh);
    if (!((v ^ c0) & m0) && (L <= 4 || lit_eq(r + p + 4, c + 1, L - 4))) return p + L;
    if (++sh == 4) {
      sh = 0;
      lo = hi;
      ++w;
      hi = *(w + 1 <= last ? w + 1 : last);
    }
  }
  return kNo;
}

HD bool seg_is_literal(const uint32_t *seg) { return seg[1] == 1 && !seg[2] && !seg[3]; }

// leftmost match of the segment in [cur, end): where it ends, or kNo
template <bool WILD, bool UTF8>
HD uint32_t seg_find(const uint8_t *r, uint32_t cur, uint32_t end, const uint32_t *cs,
                     const uint32_t *seg) {
  if (!WILD || seg_is_literal(seg)) return lit_find(r, cur, end, cs + seg[4] / 4, seg[5]);
  const uint32_t minb = seg[0];
  uint32_t hit = kNo;
  for (uint32_t p = cur; hit == kNo && end - p >= minb; ++p) {
    hit = seg_fwd<WILD, UTF8>(r, p, end, cs, seg);
    if (p == end) break;
  }
  return hit;
}

// what is left once the anchored ends are matched: segments [first, last)
// to be found in [cur, end)
struct Mid {
  uint32_t cur, end, first, last;
};

// length reject, head, tail: -1 no match, 1 match, 0 the middle decides
template <bool WILD, bool UTF8>
HD int like_ends(const uint8_t *r, uint32_t len, const uint32_t *cs, const uint32_t *of,
                 const uint32_t *pat, Mid &m) {
  const uint32_t fl = pat[0], nseg = pat[2];
  m.cur = 0;
  m.end = len;
  m.first = 0;
  m.last = nseg;
  if (len < pat[1]) return -1;
  if (!nseg) return (fl & STROM_LIKE_HEAD) && len ? -1 : 1;
  if (fl & STROM_LIKE_HEAD) {
    m.cur = seg_fwd<WILD, UTF8>(r, 0, len, cs, of + pat[3]);
    if (m.cur == kNo) return -1;
    m.first = 1;
    if (nseg == 1 && (fl & STROM_LIKE_TAIL)) return m.cur == len ? 1 : -1;
  }
  if (fl & STROM_LIKE_TAIL) {
    m.end = seg_bwd<WILD, UTF8>(r, len, m.cur, cs, of + pat[3 + nseg - 1]);
    if (m.end == kNo) return -1;
    --m.last;
  }
  return m.first == m.last ? 1 : 0;
}

// one row against the patterns from the first on, by one lane: 1 a pattern
// matches, 0 none does, -1 pattern `from` has to search more than long_row
// bytes for its middle segments: the wave takes the row over from there
template <bool WILD, bool UTF8>
HD int like_any(const uint8_t *r, uint32_t len, const uint32_t *cs, const uint32_t *of,
                uint32_t npat, uint32_t long_row, uint32_t &from) {
  for (uint32_t k = 0; k < npat; ++k) {
    const uint32_t *pat = of + of[k];
    Mid m;
    const int d = like_ends<WILD, UTF8>(r, len, cs, of, pat, m);
    if (d > 0) return 1;
    if (d < 0) continue;
    if (m.end - m.cur > long_row) {
      from = k;
      return -1;
    }
    for (uint32_t s = m.first; s < m.last && m.cur != kNo; ++s)
      m.cur = seg_find<WILD, UTF8>(r, m.cur, m.end, cs, of + pat[3 + s]);
    if (m.cur != kNo) return 1;
  }
  return 0;
}

// a malformed offset pair (file data) never matches and is never followed
template <typename OT>
HD bool row_span(const strom_qual_batch &b, uint64_t i, const uint8_t *&r, uint32_t &len) {
  const int64_t s = (int64_t)((const OT *)b.values)[i];
  const int64_t e = (int64_t)((const OT *)b.values)[i + 1];
  if (s < 0 || e < s || (uint64_t)e > b.aux_len) return false;
  r = (const uint8_t *)b.aux + s;
  len = (uint32_t)(e - s);
  return true;
}

#if defined(__HIPCC__)
// one long row by the whole wave (every lane calls it with the same row): a
// searched segment's 64 next candidate positions, one per lane
template <bool WILD, bool UTF8>
__device__ bool like_any_wave(const uint8_t *r, uint32_t len, const uint32_t *cs,
                              const uint32_t *of, uint32_t npat, uint32_t from, uint32_t lane) {
  bool h = false;
  for (uint32_t k = from; k < npat && !h; ++k) {
    const uint32_t *pat = of + of[k];
    Mid m;
    const int d = like_ends<WILD, UTF8>(r, len, cs, of, pat, m);   // uniform
    bool ok = d >= 0;
    for (uint32_t s = m.first; d == 0 && ok && s < m.last; ++s) {
      const uint32_t *seg = of + pat[3 + s];
      const uint32_t minb = seg[0];
      uint32_t found = kNo;
      for (uint32_t base = m.cur; found == kNo && m.end - base >= minb; base += 64) {
        const uint32_t p = base + lane;
        uint32_t e = kNo;
        if (p <= m.end && m.end - p >= minb) e = seg_fwd<WILD, UTF8>(r, p, m.end, cs, seg);
        const uint64_t b = __ballot(e != kNo);
        if (b) found = (uint32_t)__shfl((int)e, (int)(__ffsll((unsigned long long)b) - 1), 64);
        if (m.end - base < 64) break;
      }
      ok = found != kNo;
      m.cur = found;
    }
    h = ok;
  }
  return h;
}

template <typename OT, bool WILD, bool UTF8>
__global__ __launch_bounds__(256) void like_kernel(strom_col_qual q,
                                                   const strom_qual_batch *__restrict__ bt,
                                                   uint32_t nb, uint64_t nwords,
                                                   uint64_t *__restrict__ bitmap,
                                                   const uint64_t *__restrict__ or_src, int and_dst,
                                                   unsigned long long *__restrict__ count,
                                                   uint32_t long_row) {
  extern __shared__ __attribute__((aligned(16))) uint32_t qs[];
  __shared__ uint32_t wave_cnt[4];
  const uint32_t lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  // operands -> LDS: the literal bytes, then the pattern / segment records
  const uint32_t cw = (uint32_t)(q.const_bytes / 4), ow = (uint32_t)(q.offs_bytes / 4);
  for (uint32_t k = threadIdx.x; k < cw; k += 256) qs[k] = ((const uint32_t *)q.consts)[k];
  for (uint32_t k = threadIdx.x; k < ow; k += 256) qs[cw + k] = ((const uint32_t *)q.offs)[k];
  __syncthreads();
  const uint32_t *cs = qs, *of = qs + cw;
  const bool neg = q.flags & STROM_QUAL_NEGATE;
  uint32_t local = 0;
  const uint64_t step = (uint64_t)gridDim.x * 4;
  for (uint64_t w = (uint64_t)blockIdx.x * 4 + wid; w < nwords; w += step) {
    uint32_t lo = 0, hi = nb;
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (bt[mid].word_base <= w) lo = mid;
      else hi = mid;
    }
    const strom_qual_batch &b = bt[lo];
    const uint64_t k = w - b.word_base;
    const uint64_t i = k * 64 + lane;
    const uint64_t vword = b.valid && k * 64 < b.nrows ? ((const uint64_t *)b.valid)[k] : ~0ull;
    // per lane: its row, unless null (no form selects it) or malformed,
    // up to a search of more than long_row bytes
    bool hit = false, lng = false;
    uint32_t from = 0;
    const bool live = i < b.nrows && ((vword >> lane) & 1);
    if (live) {
      const uint8_t *r = nullptr;
      uint32_t len = 0;
      if (row_span<OT>(b, i, r, len)) {
        const int d = like_any<WILD, UTF8>(r, len, cs, of, q.nconst, long_row, from);
        lng = d < 0;
        hit = (d > 0) != neg;
      }
    }
    // per wave: the rows set aside, one after the other (the loop is uniform)
    uint64_t todo = __ballot(lng);
    while (todo) {
      const uint32_t src = (uint32_t)__ffsll((unsigned long long)todo) - 1;
      todo &= todo - 1;
      const uint8_t *r = nullptr;
      uint32_t len = 0;
      (void)row_span<OT>(b, k * 64 + src, r, len);   // checked by its lane above
      const uint32_t kf = (uint32_t)__shfl((int)from, (int)src, 64);
      const bool h = like_any_wave<WILD, UTF8>(r, len, cs, of, q.nconst, kf, lane);
      if (lane == src) hit = h != neg;
    }
    uint64_t word = __ballot(hit) & vword;
    if (or_src) word |= or_src[w];
    if (and_dst) word &= bitmap[w];
    if (lane == 0) bitmap[w] = word;
    local += __popcll(word);
  }
  if (lane == 0) wave_cnt[wid] = local;
  __syncthreads();
  if (threadIdx.x == 0)
    atomicAdd(count, (unsigned long long)(wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3]));
}
#endif

// the host's stand-in for like_any_wave: the ballot is a loop over the lanes
template <bool WILD, bool UTF8>
bool like_any_wave_host(const uint8_t *r, uint32_t len, const uint32_t *cs, const uint32_t *of,
                        uint32_t npat, uint32_t from) {
  bool h = false;
  for (uint32_t k = from; k < npat && !h; ++k) {
    const uint32_t *pat = of + of[k];
    Mid m;
    const int d = like_ends<WILD, UTF8>(r, len, cs, of, pat, m);
    bool ok = d >= 0;
    for (uint32_t s = m.first; d == 0 && ok && s < m.last; ++s) {
      const uint32_t *seg = of + pat[3 + s];
      const uint32_t minb = seg[0];
      uint32_t found = kNo;
      for (uint32_t base = m.cur; found == kNo && m.end - base >= minb; base += 64) {
        for (uint32_t lane = 0; lane < 64 && found == kNo; ++lane) {
          const uint32_t p = base + lane;
          if (p <= m.end && m.end - p >= minb) found = seg_fwd<WILD, UTF8>(r, p, m.end, cs, seg);
        }
        if (m.end - base < 64) break;
      }
      ok = found != kNo;
      m.cur = found;
    }
    h = ok;
  }
  return h;
}

template <typename OT, bool WILD, bool UTF8>
void like_host(const strom_col_qual &q, const strom_qual_batch *bt, uint32_t nb, uint64_t nwords,
               uint64_t *bitmap, const uint64_t *or_src, int and_dst, uint64_t *count,
               uint32_t long_row) {
  const uint32_t *cs = (const uint32_t *)q.consts, *of = (const uint32_t *)q.offs;
  const bool neg = q.flags & STROM_QUAL_NEGATE;
  for (uint64_t w = 0; w < nwords; ++w) {
    uint32_t lo = 0, hi = nb;
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (bt[mid].word_base <= w) lo = mid;
      else hi = mid;
    }
    const strom_qual_batch &b = bt[lo];
    const uint64_t k = w - b.word_base;
    const uint64_t vword = b.valid && k * 64 < b.nrows ? ((const uint64_t *)b.valid)[k] : ~0ull;
    uint64_t word = 0;
    for (uint32_t lane = 0; lane < 64; ++lane) {
      const uint64_t i = k * 64 + lane;
      if (i >= b.nrows || !((vword >> lane) & 1)) continue;
      const uint8_t *r = nullptr;
      uint32_t len = 0;
      if (!row_span<OT>(b, i, r, len)) continue;
      uint32_t from = 0;
      const int d = like_any<WILD, UTF8>(r, len, cs, of, q.nconst, long_row, from);
      const bool h = d < 0 ? like_any_wave_host<WILD, UTF8>(r, len, cs, of, q.nconst, from) : d > 0;
      if (h != neg) word |= 1ull << lane;
    }
    if (or_src) word |= or_src[w];
    if (and_dst) word &= bitmap[w];
    bitmap[w] = word;
    *count += (uint64_t)__builtin_popcountll(word);
  }
}

// every record inside offs, every piece inside consts (host memory only)
bool operands_ok(const strom_col_qual &q) {
  const uint32_t *of = (const uint32_t *)q.offs;
  const uint64_t ow = q.offs_bytes / 4;
  const bool wild = q.flags & STROM_QUAL_LIKE_WILD;
  if (q.nconst > ow) return false;
  for (uint32_t k = 0; k < q.nconst; ++k) {
    const uint64_t pi = of[k];
    if (pi + 3 > ow) return false;
    const uint64_t nseg = of[pi + 2];
    if (nseg > ow || pi + 3 + nseg > ow) return false;
    for (uint64_t s = 0; s < nseg; ++s) {
      const uint64_t si = of[pi + 3 + s];
      if (si + 3 > ow) return false;
      const uint64_t np = of[si + 1];
      if (np > ow || si + 3 + 3 * np > ow) return false;
      if (!wild && (np != 1 || of[si + 2])) return false;
      for (uint64_t j = 0; j < np; ++j) {
        const uint32_t *pc = of + si + 3 + 3 * j;
        if (!pc[2] || (pc[1] & 3) || (uint64_t)pc[1] + pc[2] > q.const_bytes) return false;
        if (!wild && pc[0]) return false;
      }
    }
  }
  return true;
}

uint32_t long_row_threshold() {
  static const uint32_t v = [] {
    const char *s = getenv("STROM_LIKE_LONG_ROW");
    if (!s || !*s) return (uint32_t)STROM_LIKE_LONG_ROW;
    const unsigned long long x = strtoull(s, nullptr, 10);
    return x > 0xffffffffull ? 0xffffffffu : (uint32_t)x;
  }();
  return v;
}

bool args_ok(const strom_col_qual *q, const strom_qual_batch *bt, const uint64_t *bm,
             const uint64_t *cnt) {
  if (!q || !bt || !bm || !cnt || ((uintptr_t)bm & 7)) return false;
  if (q->op != STROM_QOP_STR_LIKE || (q->type != STROM_COL_STR32 && q->type != STROM_COL_STR64))
    return false;
  if (!q->consts || !q->offs || ((q->consts | q->offs | q->const_bytes | q->offs_bytes) & 3))
    return false;
  return q->offs_bytes >= 4ull * q->nconst && q->const_bytes + q->offs_bytes <= (64u << 10);
}

#if defined(__HIPCC__)
template <typename OT, bool WILD, bool UTF8>
int launch_like(const strom_col_qual &q, const strom_qual_batch *bt, uint32_t nb, uint64_t nwords,
                uint64_t *bm, const uint64_t *orv, int and_dst, uint64_t *cnt, hipStream_t st) {
  const uint64_t g = (nwords + 3) / 4;
  const uint32_t grid = (uint32_t)(g > 8192 ? 8192 : (g ? g : 1));
  const size_t lds = (size_t)(q.const_bytes + q.offs_bytes);
  hipLaunchKernelGGL((like_kernel<OT, WILD, UTF8>), dim3(grid), dim3(256), lds, st, q, bt, nb, nwords,
                     bm, orv, and_dst, (unsigned long long *)cnt, long_row_threshold());
  return hipGetLastError() == hipSuccess ? 0 : -5;
}
#endif

}  // namespace

#define LIKE_DISPATCH(FN, ...)                                                      \
  do {                                                                              \
    const bool wild = q->flags & STROM_QUAL_LIKE_WILD;                              \
    const bool utf8 = q->flags & STROM_QUAL_LIKE_UTF8;                              \
    if (q->type == STROM_COL_STR32) {                                               \
      if (!wild) return FN<int32_t, false, false>(__VA_ARGS__);                     \
      return utf8 ? FN<int32_t, true, true>(__VA_ARGS__) : FN<int32_t, true, false>(__VA_ARGS__); \
    }                                                                               \
    if (!wild) return FN<int64_t, false, false>(__VA_ARGS__);                       \
    return utf8 ? FN<int64_t, true, true>(__VA_ARGS__) : FN<int64_t, true, false>(__VA_ARGS__);   \
  } while (0)

// STROM_QOP_STR_LIKE of strom_column_qual (colfilter.hip checks the common
// arguments and hands the launch over)
extern "C" int strom_column_like(const strom_col_qual *q, const strom_qual_batch *d_batches,
                                 uint32_t nbatches, uint64_t nwords, uint64_t *d_bitmap,
                                 const uint64_t *d_or, int and_dst, uint64_t *d_count,
                                 void *stream) {
  if (!nbatches || !nwords) return 0;
  if (!args_ok(q, d_batches, d_bitmap, d_count)) return -22;
  hipStream_t st = (hipStream_t)stream;
  LIKE_DISPATCH(launch_like, *q, d_batches, nbatches, nwords, d_bitmap, d_or, and_dst, d_count, st);
}

namespace {
template <typename OT, bool WILD, bool UTF8>
int run_host(const strom_col_qual &q, const strom_qual_batch *bt, uint32_t nb, uint64_t nwords,
             uint64_t *bm, const uint64_t *orv, int and_dst, uint64_t *cnt) {
  like_host<OT, WILD, UTF8>(q, bt, nb, nwords, bm, orv, and_dst, cnt, long_row_threshold());
  return 0;
}
}  // namespace

extern "C" int strom_column_like_host(const strom_col_qual *q, const strom_qual_batch *batches,
                                      uint32_t nbatches, uint64_t nwords, uint64_t *bitmap,
                                      const uint64_t *or_src, int and_dst, uint64_t *count) {
  if (!nbatches || !nwords) return 0;
  if (!args_ok(q, batches, bitmap, count) || !operands_ok(*q)) return -22;
  LIKE_DISPATCH(run_host, *q, batches, nbatches, nwords, bitmap, or_src, and_dst, count);
}
