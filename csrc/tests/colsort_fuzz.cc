// Randomized test of the radix sort's host copy (csrc/kernels/colsort.hip,
// strom_sort_*_host), built host-only with ASan + UBSan (make
// build/colsort_fuzz).  Each iteration draws a row count around the tile
// boundaries, one to four order columns of random storage types, directions
// and validity, values from small pools (heavy ties, the types' extremes,
// +-0.0, infinities, denormals, NaNs of several payloads) or random bits, and
// sorts them with the schedule of passes the device runs; the permutation is
// compared with std::stable_sort under a comparator written here.  Then the
// gather: every width, validity, a string column's lengths and characters, a
// random first / count window, and permutation entries planted out of range,
// against a per-row loop, with the exact error count.  A few hand-built
// inputs and the refusals come first.
//
// Every buffer is its own heap block of exactly the bytes the contract names,
// so a read or a write past one is an ASan report.
//
//   colsort_fuzz ITERATIONS [SEED]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <numeric>
#include <random>
#include <vector>

#include "strom/strom.h"

namespace {

std::mt19937_64 rng;
uint32_t rnd(uint32_t n) { return n ? (uint32_t)(rng() % n) : 0; }

#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__); \
      fprintf(stderr, __VA_ARGS__);                        \
      fprintf(stderr, "\n");                               \
      exit(1);                                             \
    }                                                      \
  } while (0)

// an exact-size heap block (at least one byte, so that it has an address)
template <typename T> struct Block {
  std::unique_ptr<T[]> mem;
  size_t n = 0;
  explicit Block(size_t count = 0) { reset(count); }
  void reset(size_t count) {
    n = count;
    mem.reset(new T[count ? count : 1]());
  }
  T *p() const { return mem.get(); }
  T &operator[](size_t i) const { return mem[i]; }
};

const int kTypes[] = {STROM_COL_I8, STROM_COL_I16, STROM_COL_I32, STROM_COL_I64, STROM_COL_U8,
                      STROM_COL_U16, STROM_COL_U32, STROM_COL_U64, STROM_COL_F32, STROM_COL_F64};

uint32_t width_of(int type) {
  switch (type) {
    case STROM_COL_I8: case STROM_COL_U8: return 1;
    case STROM_COL_I16: case STROM_COL_U16: return 2;
    case STROM_COL_I32: case STROM_COL_U32: case STROM_COL_F32: return 4;
    default: return 8;
  }
}

bool is_float(int type) { return type == STROM_COL_F32 || type == STROM_COL_F64; }

struct Col {
  int type = 0;
  bool desc = false, has_valid = false;
  Block<uint8_t> raw, valid;
};

template <typename T> T at(const Col &c, uint64_t i) {
  T x;
  memcpy(&x, c.raw.p() + i * sizeof(T), sizeof(T));
  return x;
}

// value / NaN / null
template <typename T> int cls_of(const Col &c, uint64_t i) {
  if (c.has_valid && !c.valid[i]) return 2;
  const T x = at<T>(c, i);
  return x != x ? 1 : 0;
}

template <typename T> int cmp_t(const Col &c, uint64_t a, uint64_t b) {
  const int ca = cls_of<T>(c, a), cb = cls_of<T>(c, b);
  if (ca != cb) return ca < cb ? -1 : 1;
  if (ca) return 0;
  const T x = at<T>(c, a), y = at<T>(c, b);
  if (x == y) return 0;                            // -0.0 == +0.0
  return ((x < y) != c.desc) ? -1 : 1;
}

int cmp(const Col &c, uint64_t a, uint64_t b) {
  switch (c.type) {
    case STROM_COL_I8: return cmp_t<int8_t>(c, a, b);
    case STROM_COL_I16: return cmp_t<int16_t>(c, a, b);
    case STROM_COL_I32: return cmp_t<int32_t>(c, a, b);
    case STROM_COL_I64: return cmp_t<int64_t>(c, a, b);
    case STROM_COL_U8: return cmp_t<uint8_t>(c, a, b);
    case STROM_COL_U16: return cmp_t<uint16_t>(c, a, b);
    case STROM_COL_U32: return cmp_t<uint32_t>(c, a, b);
    case STROM_COL_U64: return cmp_t<uint64_t>(c, a, b);
    case STROM_COL_F32: return cmp_t<float>(c, a, b);
    default: return cmp_t<double>(c, a, b);
  }
}

const uint64_t kF64[] = {0x0000000000000000ull, 0x8000000000000000ull, 0x7ff0000000000000ull,
                         0xfff0000000000000ull, 0x0000000000000001ull, 0x8000000000000001ull,
                         0x7ff8000000000000ull, 0x7ff8000000000001ull, 0xfff8000000001234ull,
                         0x3ff0000000000000ull, 0xbff0000000000000ull, 0x7fefffffffffffffull};
const uint32_t kF32[] = {0x00000000u, 0x80000000u, 0x7f800000u, 0xff800000u, 0x00000001u,
                         0x80000001u, 0x7fc00000u, 0x7fc00001u, 0xffc01234u, 0x3f800000u,
                         0xbf800000u, 0x7f7fffffu};

void fill(Col &c, uint64_t n) {
  const uint32_t w = width_of(c.type);
  c.raw.reset(n * w);
  const uint32_t mode = rnd(4);                    // random bits / pool / one byte / nearly equal
  const uint32_t byte = rnd(w);
  for (uint64_t i = 0; i < n; ++i) {
    uint64_t bits = rng();
    if (mode == 1) {
      if (c.type == STROM_COL_F64) bits = kF64[rnd(12)];
      else if (c.type == STROM_COL_F32) bits = kF32[rnd(12)];
      else {
        const uint64_t pool[] = {0, 1, ~0ull, 1ull << (8 * w - 1), (1ull << (8 * w - 1)) - 1, 255,
                                 256, 65535, 65536};
        bits = pool[rnd(9)];
      }
    } else if (mode == 2) {
      bits = 0x0101010101010101ull ^ ((uint64_t)rnd(256) << (8 * byte));
    } else if (mode == 3) {
      bits = rnd(100) ? 42 : rng();
    }
    memcpy(c.raw.p() + i * w, &bits, w);
  }
  c.has_valid = rnd(3) == 0;
  c.valid.reset(c.has_valid ? n : 0);
  const uint32_t share = rnd(3) == 0 ? 100 : 10;
  for (uint64_t i = 0; c.has_valid && i < n; ++i) c.valid[i] = rnd(100) >= share;
}

// the device's schedule over the host copies; returns the permutation
std::vector<uint32_t> sort_host(const std::vector<Col> &cols, uint64_t n) {
  Block<uint64_t> key[2] = {Block<uint64_t>(n), Block<uint64_t>(n)};
  Block<uint32_t> perm[2] = {Block<uint32_t>(n), Block<uint32_t>(n)};
  Block<uint32_t> work(strom_sort_work_bytes(n) / 4);
  int cur = 0;
  uint32_t first = STROM_SORT_FIRST;
  auto pass = [&](uint32_t shift) {
    CHECK(strom_sort_pass_host(key[cur].p(), perm[cur].p(), key[1 - cur].p(), perm[1 - cur].p(),
                               n, shift, work.p()) == 0, "pass");
    cur = 1 - cur;
  };
  for (size_t k = cols.size(); k-- > 0;) {
    const Col &c = cols[k];
    const uint8_t *ok = c.has_valid ? c.valid.p() : nullptr;
    CHECK(strom_sort_encode_host(c.type, first | (c.desc ? STROM_SORT_DESC : 0), c.raw.p(), ok,
                                 perm[cur].p(), n, key[cur].p()) == 0, "encode");
    first = 0;
    for (uint32_t b = 0; b < width_of(c.type); ++b) pass(8 * b);
    if (c.has_valid || is_float(c.type)) {
      CHECK(strom_sort_encode_host(c.type, STROM_SORT_CLASS, c.raw.p(), ok, perm[cur].p(), n,
                                   key[cur].p()) == 0, "class encode");
      pass(0);
    }
  }
  return std::vector<uint32_t>(perm[cur].p(), perm[cur].p() + n);
}

void check_sort(const std::vector<Col> &cols, uint64_t n, const char *what) {
  const std::vector<uint32_t> got = sort_host(cols, n);
  std::vector<uint32_t> want(n);
  std::iota(want.begin(), want.end(), 0u);
  std::stable_sort(want.begin(), want.end(), [&](uint32_t a, uint32_t b) {
    for (const Col &c : cols) {
      const int r = cmp(c, a, b);
      if (r) return r < 0;
    }
    return false;
  });
  for (uint64_t i = 0; i < n; ++i)
    CHECK(got[i] == want[i], "%s: n=%llu position %llu: %u, expected %u", what,
          (unsigned long long)n, (unsigned long long)i, got[i], want[i]);
}

uint64_t draw_n() {
  const uint64_t t = STROM_SORT_TILE;
  const uint64_t edges[] = {0, 1, 2, 63, 64, 65, 511, 512, 513, t - 1, t, t + 1, 2 * t, 3 * t + 17};
  return rnd(3) ? edges[rnd(14)] : rnd(3 * (uint32_t)t);
}

void fuzz_sort() {
  const uint64_t n = draw_n();
  std::vector<Col> cols(1 + rnd(4));
  for (Col &c : cols) {
    c.type = kTypes[rnd(10)];
    c.desc = rnd(2);
    fill(c, n);
  }
  check_sort(cols, n, "fuzz");
}

void fuzz_apply() {
  const uint64_t n = rnd(2) ? rnd(600) : rnd(9000);
  Block<uint32_t> perm(n);
  std::iota(perm.p(), perm.p() + n, 0u);
  std::shuffle(perm.p(), perm.p() + n, rng);
  uint64_t first = rnd(3) ? rnd((uint32_t)n + 1) : (rnd(2) ? 0 : n + rnd(5));
  uint64_t count = rnd(3) ? rnd((uint32_t)n + 2) : n + rnd(7);
  const uint64_t f = std::min(first, n), cnt = std::min(count, n - f);
  uint64_t bad = 0;
  for (uint64_t i = 0; i < n; ++i)
    if (rnd(50) == 0) {
      perm[i] = (uint32_t)n + rnd(3) * 1000u + (rnd(2) ? 0u : 0xfff00000u);
      if (i >= f && i < f + cnt) ++bad;
    }
  Block<int64_t> rows_in(n), rows_out(cnt);
  for (uint64_t i = 0; i < n; ++i) rows_in[i] = (int64_t)rng();
  const uint32_t widths[] = {1, 2, 4, 8, 16};
  const uint32_t ncols = rnd(STROM_SORT_MAX_COLS + 1);
  std::vector<strom_sort_col> cols(ncols);
  std::vector<Block<uint8_t>> in(ncols), out(ncols), vin(ncols), vout(ncols);
  std::vector<Block<int64_t>> sin(ncols), sout(ncols);
  for (uint32_t k = 0; k < ncols; ++k) {
    strom_sort_col &c = cols[k];
    memset(&c, 0, sizeof c);
    const bool hv = rnd(2), ov = hv || rnd(4) == 0;
    if (hv) {
      vin[k].reset(n);
      for (uint64_t i = 0; i < n; ++i) vin[k][i] = rnd(2);
      c.in_valid = (uint64_t)(uintptr_t)vin[k].p();
    }
    if (ov) {
      vout[k].reset(cnt);
      memset(vout[k].p(), 0xAB, cnt);
      c.out_valid = (uint64_t)(uintptr_t)vout[k].p();
    }
    if (rnd(4) == 0) {
      c.kind = STROM_SORT_LEN;
      sin[k].reset(n + 1);
      int64_t run = rnd(5);
      for (uint64_t i = 0; i <= n; ++i) {
        sin[k][i] = run;
        run += rnd(9);
      }
      if (n && rnd(4) == 0) sin[k][rnd((uint32_t)n + 1)] = rnd(2) ? -3 : 1 << 20;   // malformed
      sout[k].reset(cnt);
      c.in = (uint64_t)(uintptr_t)sin[k].p();
      c.out = (uint64_t)(uintptr_t)sout[k].p();
    } else {
      c.kind = STROM_SORT_FIXED;
      c.width = widths[rnd(5)];
      in[k].reset(n * c.width);
      out[k].reset(cnt * c.width);
      for (uint64_t i = 0; i < n * c.width; ++i) in[k][i] = (uint8_t)rng();
      memset(out[k].p(), 0xCD, cnt * c.width);
      c.in = (uint64_t)(uintptr_t)in[k].p();
      c.out = (uint64_t)(uintptr_t)out[k].p();
    }
  }
  uint64_t err = 5;
  CHECK(strom_sort_apply_host(perm.p(), n, first, count, rows_in.p(), rows_out.p(),
                              ncols ? cols.data() : nullptr, ncols, &err) == 0, "apply");
  CHECK(err == 5 + bad, "apply: %llu errors, expected %llu", (unsigned long long)(err - 5),
        (unsigned long long)bad);
  for (uint64_t i = 0; i < cnt; ++i) {
    const uint64_t p = perm[f + i];
    const bool ok = p < n;
    CHECK(rows_out[i] == (ok ? rows_in[p] : 0), "apply: row id %llu", (unsigned long long)i);
    for (uint32_t k = 0; k < ncols; ++k) {
      const strom_sort_col &c = cols[k];
      if (c.out_valid)
        CHECK(vout[k][i] == (ok ? (c.in_valid ? vin[k][p] : 1) : 0), "apply: validity");
      if (c.kind == STROM_SORT_FIXED) {
        for (uint32_t b = 0; b < c.width; ++b)
          CHECK(out[k][i * c.width + b] == (ok ? in[k][p * c.width + b] : 0), "apply: column %u", k);
      } else {
        int64_t len = 0;
        if (ok && sin[k][p] >= 0 && sin[k][p + 1] > sin[k][p]) len = sin[k][p + 1] - sin[k][p];
        CHECK(sout[k][i] == len, "apply: length of column %u row %llu", k, (unsigned long long)i);
      }
    }
  }
  // the characters of each string column behind its lengths' prefix
  for (uint32_t k = 0; k < ncols; ++k) {
    if (cols[k].kind != STROM_SORT_LEN || !cnt) continue;
    uint64_t in_len = 0;
    for (uint64_t i = 0; i <= n; ++i)
      if (sin[k][i] > 0 && sin[k][i] < (1 << 19)) in_len = std::max<uint64_t>(in_len, sin[k][i]);
    Block<uint8_t> chars(in_len);
    for (uint64_t i = 0; i < in_len; ++i) chars[i] = (uint8_t)(1 + rnd(255));
    Block<int64_t> off(cnt + 1);
    for (uint64_t i = 0; i < cnt; ++i) off[i + 1] = off[i] + sout[k][i];
    const uint64_t total = (uint64_t)off[cnt];
    // whole dwords need 4-byte alignment: new[] gives 16
    Block<uint8_t> oc(total);
    memset(oc.p(), 0xEE, total);
    CHECK(strom_sort_chars_host(perm.p(), n, first, count, sin[k].p(), chars.p(), in_len, off.p(),
                                oc.p(), total) == 0, "chars");
    for (uint64_t i = 0; i < cnt; ++i) {
      const uint64_t p = perm[f + i];
      for (int64_t j = 0; j < sout[k][i]; ++j) {
        const uint64_t src = (uint64_t)sin[k][p] + j;
        CHECK(oc[off[i] + j] == (src < in_len ? chars[src] : 0), "chars: column %u row %llu", k,
              (unsigned long long)i);
      }
    }
  }
}

void hand_built() {
  // all equal: the identity; one row; none
  for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)STROM_SORT_TILE + 3}) {
    std::vector<Col> cols(1);
    cols[0].type = STROM_COL_I64;
    cols[0].raw.reset(n * 8);
    const std::vector<uint32_t> got = sort_host(cols, n);
    for (uint64_t i = 0; i < n; ++i) CHECK(got[i] == i, "all equal: not the identity");
  }
  // -0.0 and +0.0 tie, NaNs of any payload tie behind the values, nulls last,
  // in both directions
  for (int desc = 0; desc < 2; ++desc) {
    std::vector<Col> cols(1);
    Col &c = cols[0];
    c.type = STROM_COL_F64;
    c.desc = desc;
    const uint64_t v[] = {0x7ff8000000000001ull, 0x8000000000000000ull, 0x3ff0000000000000ull,
                          0x0000000000000000ull, 0xfff8000000000000ull, 0xbff0000000000000ull,
                          0x4000000000000000ull};
    c.raw.reset(sizeof v);
    memcpy(c.raw.p(), v, sizeof v);
    c.has_valid = true;
    c.valid.reset(7);
    memset(c.valid.p(), 1, 7);
    c.valid[6] = 0;
    const uint32_t asc[] = {5, 1, 3, 2, 0, 4, 6}, dsc[] = {2, 1, 3, 5, 0, 4, 6};
    const std::vector<uint32_t> got = sort_host(cols, 7);
    for (int i = 0; i < 7; ++i) CHECK(got[i] == (desc ? dsc : asc)[i], "hand-built floats");
    check_sort(cols, 7, "hand-built floats");
  }
}

void refusals() {
  Block<uint64_t> k0(8), k1(8);
  Block<uint32_t> p0(8), p1(8), work(strom_sort_work_bytes(8) / 4);
  Block<int64_t> r0(8), r1(8);
  uint64_t err = 0;
  const uint64_t big = 1ull << 32;
  CHECK(strom_sort_work_bytes(0) == 1024 && strom_sort_work_bytes(STROM_SORT_TILE + 1) == 3072,
        "work bytes");
  CHECK(strom_sort_encode_host(0, 0, r0.p(), nullptr, p0.p(), 8, k0.p()) == -22, "type 0");
  CHECK(strom_sort_encode_host(STROM_COL_BOOL, 0, r0.p(), nullptr, p0.p(), 8, k0.p()) == -22,
        "bool");
  CHECK(strom_sort_encode_host(STROM_COL_I64, 8, r0.p(), nullptr, p0.p(), 8, k0.p()) == -22,
        "flag");
  CHECK(strom_sort_encode_host(STROM_COL_I64, 0, nullptr, nullptr, p0.p(), 8, k0.p()) == -22,
        "null values");
  CHECK(strom_sort_encode_host(STROM_COL_I64, 0, r0.p(), nullptr, nullptr, 8, k0.p()) == -22,
        "null perm");
  CHECK(strom_sort_encode_host(STROM_COL_I64, 0, r0.p(), nullptr, p0.p(), 8, nullptr) == -22,
        "null key");
  CHECK(strom_sort_encode_host(STROM_COL_I64, 0, r0.p(), nullptr, p0.p(), big, k0.p()) == -22,
        "n 2^32");
  CHECK(strom_sort_encode_host(STROM_COL_I64, 0, r0.p(), nullptr, p0.p(), 0, k0.p()) == 0, "n 0");
  CHECK(strom_sort_pass_host(k0.p(), p0.p(), k1.p(), p1.p(), big, 0, work.p()) == -22, "n 2^32");
  CHECK(strom_sort_pass_host(k0.p(), p0.p(), k1.p(), p1.p(), 8, 4, work.p()) == -22, "shift 4");
  CHECK(strom_sort_pass_host(k0.p(), p0.p(), k1.p(), p1.p(), 8, 64, work.p()) == -22, "shift 64");
  CHECK(strom_sort_pass_host(k0.p(), p0.p(), k0.p(), p1.p(), 8, 0, work.p()) == -22, "in place");
  CHECK(strom_sort_pass_host(nullptr, p0.p(), k1.p(), p1.p(), 8, 0, work.p()) == -22, "null");
  CHECK(strom_sort_pass_host(k0.p(), p0.p(), k1.p(), p1.p(), 8, 0, nullptr) == -22, "null work");
  CHECK(strom_sort_pass_host(k0.p(), p0.p(), k1.p(), p1.p(), 0, 0, work.p()) == 0, "n 0");
  strom_sort_col c;
  memset(&c, 0, sizeof c);
  c.kind = STROM_SORT_FIXED;
  c.width = 8;
  c.in = (uint64_t)(uintptr_t)r0.p();
  c.out = (uint64_t)(uintptr_t)r1.p();
  std::vector<strom_sort_col> many(STROM_SORT_MAX_COLS + 1, c);
  CHECK(strom_sort_apply_host(p0.p(), 8, 0, 8, nullptr, nullptr, many.data(),
                              STROM_SORT_MAX_COLS + 1, &err) == -22, "17 columns");
  CHECK(strom_sort_apply_host(nullptr, 8, 0, 8, nullptr, nullptr, &c, 1, &err) == -22, "null perm");
  CHECK(strom_sort_apply_host(p0.p(), 8, 0, 8, nullptr, nullptr, &c, 1, nullptr) == -22, "null err");
  CHECK(strom_sort_apply_host(p0.p(), 8, 0, 8, r0.p(), nullptr, &c, 1, &err) == -22, "half rows");
  CHECK(strom_sort_apply_host(p0.p(), 8, 0, 8, nullptr, nullptr, nullptr, 1, &err) == -22,
        "null cols");
  CHECK(strom_sort_apply_host(p0.p(), big, 0, 8, nullptr, nullptr, &c, 1, &err) == -22, "n 2^32");
  for (uint32_t w : {0u, 3u, 5u, 32u}) {
    strom_sort_col b = c;
    b.width = w;
    CHECK(strom_sort_apply_host(p0.p(), 8, 0, 8, nullptr, nullptr, &b, 1, &err) == -22, "width");
  }
  for (uint32_t kind : {0u, 3u}) {
    strom_sort_col b = c;
    b.kind = kind;
    CHECK(strom_sort_apply_host(p0.p(), 8, 0, 8, nullptr, nullptr, &b, 1, &err) == -22, "kind");
  }
  strom_sort_col b = c;
  b.out = 0;
  CHECK(strom_sort_apply_host(p0.p(), 8, 0, 8, nullptr, nullptr, &b, 1, &err) == -22, "null out");
  CHECK(strom_sort_chars_host(p0.p(), 8, 0, 8, nullptr, (const uint8_t *)r0.p(), 8, r1.p(),
                              (uint8_t *)k0.p(), 8) == -22, "null offsets");
  CHECK(err == 0, "a refused call counted an error");
}

}  // namespace

int main(int argc, char **argv) {
  const long iters = argc > 1 ? atol(argv[1]) : 300;
  rng.seed(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1);
  refusals();
  hand_built();
  for (long i = 0; i < iters; ++i) {
    fuzz_sort();
    fuzz_apply();
  }
  printf("%ld iterations ok\n", iters);
  return 0;
}
