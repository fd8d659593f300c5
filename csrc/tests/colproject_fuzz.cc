// Randomized test of the select-list walk's host copy (csrc/kernels/
// colproject.hip, strom_bitmap_to_rows_multi_host), built host-only with
// ASan + UBSan (make build/colproject_fuzz).  Each iteration draws a split of
// rows into record batches (every batch on fresh bitmap words, now and then
// empty words between two batches), a bitmap (dense, sparse, whole words,
// bits past a batch's rows), one to sixteen columns of every kind and width
// with validity on some batches only, string columns whose offset pairs are
// now and then negative, decreasing or past the character buffer, and
// cursors that do not start at zero.  The results are compared bit for bit
// with a per-row loop written here.
//
// Every input buffer is allocated at exactly the bytes its batch holds and
// every output at exactly the bytes the final cursors name, each its own
// heap block and at an odd address where the contract allows one, so a read
// or a write past one is an ASan report.
//
//   colproject_fuzz ITERATIONS [SEED]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <random>
#include <vector>

#include "strom/strom.h"

namespace {

std::mt19937_64 rng;
uint32_t rnd(uint32_t n) { return n ? (uint32_t)(rng() % n) : 0; }

// an exact-size heap block, its first byte `skew` bytes into the allocation
struct Block {
  std::unique_ptr<uint8_t[]> mem;
  uint8_t *p = nullptr;
  size_t n = 0;
  void alloc(size_t bytes, size_t align, uint8_t fill) {
    // new[] gives 16-byte alignment; the block ends where the allocation does
    const size_t skew = align >= 16 ? 0 : (16 - bytes % 16) % 16 / align * align;
    mem.reset(new uint8_t[skew + bytes]);
    p = mem.get() + skew;
    n = bytes;
    memset(p, fill, bytes);
  }
};

struct Col {
  int kind;
  uint32_t width;
  bool want_valid;
  std::vector<Block> values, valid, aux;       // per batch
  std::vector<bool> has_valid;
  std::vector<strom_qual_batch> table;
};

bool get_bit(const uint8_t *p, uint64_t i) { return (p[i >> 3] >> (i & 7)) & 1; }

int64_t load_off(const Col &c, uint32_t b, uint64_t r) {
  if (c.kind == STROM_PROJ_STR64) {
    int64_t v;
    memcpy(&v, c.values[b].p + 8 * r, 8);
    return v;
  }
  int32_t v;
  memcpy(&v, c.values[b].p + 4 * r, 4);
  return v;
}

void store_off(Col &c, uint32_t b, uint64_t r, int64_t v) {
  if (c.kind == STROM_PROJ_STR64) memcpy(c.values[b].p + 8 * r, &v, 8);
  else {
    const int32_t x = (int32_t)v;
    memcpy(c.values[b].p + 4 * r, &x, 4);
  }
}

int fail(uint64_t it, const char *what) {
  fprintf(stderr, "iteration %llu: %s\n", (unsigned long long)it, what);
  return 1;
}

int one(uint64_t it) {
  // ---- batches
  const uint32_t nb = 1 + rnd(rnd(4) ? 3 : 12);
  std::vector<strom_filter_batch> bt(nb);
  uint64_t w = rnd(4) ? 0 : rnd(3), row = rnd(1000);
  for (uint32_t b = 0; b < nb; ++b) {
    const uint32_t k = rnd(8);
    const uint64_t n = k == 0 ? 0 : k == 1 ? 1 + rnd(3) : k == 2 ? 64 * (1 + rnd(3)) : 1 + rnd(700);
    bt[b] = {0, 0, n, w, row};
    w += (n + 63) / 64 + (rnd(6) ? 0 : rnd(3));
    row += n;
  }
  const uint64_t nwords = rnd(10) ? w : (w ? rnd((uint32_t)w + 1) : 0);
  // ---- bitmap
  Block bm;
  bm.alloc(8 * nwords, 8, 0);
  const uint32_t mode = rnd(6);
  for (uint64_t i = 0; i < nwords; ++i) {
    uint64_t x = 0;
    switch (mode) {
      case 0: x = rng(); break;
      case 1: x = rng() & rng() & rng() & rng(); break;
      case 2: x = rnd(2) ? ~0ull : 0; break;
      case 3: x = 1ull << rnd(64); break;
      case 4: x = ~0ull; break;
      default: x = rnd(3) ? 0 : rng(); break;
    }
    memcpy(bm.p + 8 * i, &x, 8);
  }
  // ---- columns
  const uint32_t ncols = rnd(3) ? 1 + rnd(4) : 1 + rnd(STROM_PROJ_MAX_COLS);
  std::vector<Col> cols(ncols);
  for (Col &c : cols) {
    static const uint32_t widths[] = {1, 2, 4, 8, 16};
    const uint32_t k = rnd(8);
    c.kind = k < 4 ? STROM_PROJ_FIXED : k == 4 ? STROM_PROJ_BOOL : k < 7 ? STROM_PROJ_STR32
                                                                         : STROM_PROJ_STR64;
    c.width = c.kind == STROM_PROJ_FIXED ? widths[rnd(5)] : 0;
    c.want_valid = rnd(2);
    c.values.resize(nb);
    c.valid.resize(nb);
    c.aux.resize(nb);
    c.has_valid.resize(nb);
    c.table.resize(nb);
    for (uint32_t b = 0; b < nb; ++b) {
      const uint64_t n = bt[b].nrows;
      c.has_valid[b] = rnd(3) == 0;
      if (c.has_valid[b]) {
        c.valid[b].alloc((n + 7) / 8, 1, 0);
        for (size_t i = 0; i < c.valid[b].n; ++i) c.valid[b].p[i] = (uint8_t)rng();
      }
      uint64_t auxlen = 0;
      if (c.kind == STROM_PROJ_FIXED) {
        c.values[b].alloc(n * c.width, 1, 0);
        for (size_t i = 0; i < c.values[b].n; ++i) c.values[b].p[i] = (uint8_t)rng();
      } else if (c.kind == STROM_PROJ_BOOL) {
        c.values[b].alloc((n + 7) / 8, 1, 0);
        for (size_t i = 0; i < c.values[b].n; ++i) c.values[b].p[i] = (uint8_t)rng();
      } else {
        const uint32_t ow = c.kind == STROM_PROJ_STR64 ? 8 : 4;
        c.values[b].alloc(n ? (n + 1) * ow : 0, 1, 0);
        std::vector<int64_t> o(n + 1, 0);
        for (uint64_t r = 0; r < n; ++r)
          o[r + 1] = o[r] + (rnd(5) ? rnd(21) : rnd(40) ? 0 : 300 + rnd(5000));
        auxlen = n ? (uint64_t)o[n] : 0;
        // malformed pairs: negative, decreasing, past the buffer
        if (n && rnd(3) == 0)
          for (uint32_t t = 0, m = 1 + rnd(4); t < m; ++t) {
            const uint64_t r = rnd((uint32_t)n + 1);
            const uint32_t how = rnd(4);
            o[r] = how == 0 ? -1 - (int64_t)rnd(100) : how == 1 ? (int64_t)auxlen + 1 + rnd(100)
                 : how == 2 ? (ow == 8 ? INT64_MIN + rnd(3) : INT32_MIN + (int64_t)rnd(3))
                            : (ow == 8 ? INT64_MAX - rnd(3) : INT32_MAX - (int64_t)rnd(3));
          }
        for (uint64_t r = 0; r <= n && n; ++r) store_off(c, b, r, o[r]);
        c.aux[b].alloc(auxlen, 1, 0);
        for (size_t i = 0; i < auxlen; ++i) c.aux[b].p[i] = (uint8_t)('a' + rng() % 26);
      }
      c.table[b] = {(uint64_t)(uintptr_t)c.values[b].p,
                    c.has_valid[b] ? (uint64_t)(uintptr_t)c.valid[b].p : 0,
                    n, bt[b].word_base, bt[b].row_base,
                    (uint64_t)(uintptr_t)c.aux[b].p, auxlen};
    }
  }
  // ---- the per-row loop
  const uint64_t total0 = rnd(2) ? rnd(9) : 0;
  std::vector<int64_t> ids;
  struct Want {
    std::vector<uint8_t> vals, valid, chars;
    std::vector<int64_t> starts;
    uint64_t cur0 = 0;
  };
  std::vector<Want> want(ncols);
  for (Want &x : want) x.cur0 = rnd(2) ? rnd(7) : 0;
  for (uint64_t i = 0; i < nwords; ++i) {
    uint64_t x;
    memcpy(&x, bm.p + 8 * i, 8);
    // the batch of word i: the last one that starts at or before it
    int b = -1;
    for (uint32_t k = 0; k < nb; ++k)
      if (bt[k].word_base <= i) b = (int)k;
    if (b < 0) continue;
    for (uint32_t bit = 0; bit < 64; ++bit) {
      if (!((x >> bit) & 1)) continue;
      const uint64_t r = (i - bt[b].word_base) * 64 + bit;
      if (r >= bt[b].nrows) continue;
      ids.push_back((int64_t)(bt[b].row_base + r));
      for (uint32_t k = 0; k < ncols; ++k) {
        const Col &c = cols[k];
        Want &o = want[k];
        o.valid.push_back(c.has_valid[b] ? get_bit(c.valid[b].p, r) : 1);
        if (c.kind == STROM_PROJ_FIXED) {
          o.vals.insert(o.vals.end(), c.values[b].p + r * c.width, c.values[b].p + (r + 1) * c.width);
        } else if (c.kind == STROM_PROJ_BOOL) {
          o.vals.push_back(get_bit(c.values[b].p, r));
        } else {
          const int64_t a = load_off(c, (uint32_t)b, r), e = load_off(c, (uint32_t)b, r + 1);
          o.starts.push_back((int64_t)(o.cur0 + o.chars.size()));
          if (a >= 0 && e >= a && (uint64_t)e <= c.aux[b].n)
            o.chars.insert(o.chars.end(), c.aux[b].p + a, c.aux[b].p + e);
        }
      }
    }
  }
  // ---- exact-size outputs and the call
  const uint64_t nsel = ids.size();
  Block out, total;
  out.alloc(8 * (total0 + nsel), 8, 0xEE);
  total.alloc(8, 8, 0);
  memcpy(total.p, &total0, 8);
  std::vector<Block> o_vals(ncols), o_valid(ncols), o_chars(ncols), o_cur(ncols);
  std::vector<strom_proj_col> pc(ncols);
  for (uint32_t k = 0; k < ncols; ++k) {
    const Col &c = cols[k];
    const bool str = c.kind == STROM_PROJ_STR32 || c.kind == STROM_PROJ_STR64;
    const uint32_t per = str ? 8 : c.kind == STROM_PROJ_BOOL ? 1 : c.width;
    o_vals[k].alloc((size_t)per * (total0 + nsel), per == 16 ? 8 : per, 0xEE);
    pc[k] = {c.kind, c.width, (uint64_t)(uintptr_t)c.table.data(), (uint64_t)(uintptr_t)o_vals[k].p,
             0, 0, 0};
    if (c.want_valid) {
      o_valid[k].alloc(total0 + nsel, 1, 0xEE);
      pc[k].out_valid = (uint64_t)(uintptr_t)o_valid[k].p;
    }
    if (str) {
      o_chars[k].alloc(want[k].cur0 + want[k].chars.size(), 1, 0xEE);
      o_cur[k].alloc(8, 8, 0);
      memcpy(o_cur[k].p, &want[k].cur0, 8);
      pc[k].out_chars = (uint64_t)(uintptr_t)o_chars[k].p;
      pc[k].char_cursor = (uint64_t)(uintptr_t)o_cur[k].p;
    }
  }
  const int rc = strom_bitmap_to_rows_multi_host((const uint64_t *)bm.p, nwords, bt.data(), nb,
                                                 (int64_t *)out.p, (uint64_t *)total.p, pc.data(),
                                                 ncols);
  if (rc) return fail(it, "rc != 0");
  // ---- compare
  uint64_t got_total;
  memcpy(&got_total, total.p, 8);
  if (got_total != total0 + (nwords ? nsel : 0)) return fail(it, "row cursor");
  if (!nwords) return 0;
  for (uint64_t i = 0; i < total0 * 8; ++i)
    if (out.p[i] != 0xEE) return fail(it, "row ids before the cursor written");
  if (nsel && memcmp(out.p + 8 * total0, ids.data(), 8 * nsel)) return fail(it, "row ids");
  for (uint32_t k = 0; k < ncols; ++k) {
    const Col &c = cols[k];
    const Want &o = want[k];
    const bool str = c.kind == STROM_PROJ_STR32 || c.kind == STROM_PROJ_STR64;
    const uint32_t per = str ? 8 : c.kind == STROM_PROJ_BOOL ? 1 : c.width;
    for (uint64_t i = 0; i < total0 * per; ++i)
      if (o_vals[k].p[i] != 0xEE) return fail(it, "values before the cursor written");
    const void *exp = str ? (const void *)o.starts.data() : (const void *)o.vals.data();
    if (nsel && memcmp(o_vals[k].p + total0 * per, exp, nsel * per)) return fail(it, "values");
    if (c.want_valid) {
      for (uint64_t i = 0; i < total0; ++i)
        if (o_valid[k].p[i] != 0xEE) return fail(it, "validity before the cursor written");
      if (nsel && memcmp(o_valid[k].p + total0, o.valid.data(), nsel)) return fail(it, "validity");
    }
    if (str) {
      uint64_t cur;
      memcpy(&cur, o_cur[k].p, 8);
      if (cur != o.cur0 + o.chars.size()) return fail(it, "character cursor");
      for (uint64_t i = 0; i < o.cur0; ++i)
        if (o_chars[k].p[i] != 0xEE) return fail(it, "characters before the cursor written");
      if (!o.chars.empty() && memcmp(o_chars[k].p + o.cur0, o.chars.data(), o.chars.size()))
        return fail(it, "characters");
    }
  }
  return 0;
}

int bad_args() {
  uint64_t bm[1] = {1}, total = 0, cur = 0;
  int64_t out[1], vals[2];
  uint8_t chars[8];
  strom_filter_batch b = {0, 0, 1, 0, 0};
  int64_t v[2] = {0, 0};
  strom_qual_batch q = {(uint64_t)(uintptr_t)v, 0, 1, 0, 0, 0, 0};
  strom_proj_col c = {STROM_PROJ_FIXED, 8, (uint64_t)(uintptr_t)&q, (uint64_t)(uintptr_t)vals, 0, 0, 0};
  std::vector<strom_proj_col> many(STROM_PROJ_MAX_COLS + 1, c);
  auto call = [&](const strom_proj_col *cols, uint32_t n, uint64_t nwords = 1) {
    return strom_bitmap_to_rows_multi_host(bm, nwords, &b, 1, out, &total, cols, n);
  };
  if (call(&c, 1, 0) != 0 || total != 0) return 1;
  if (call(&c, 0) != -22 || call(many.data(), STROM_PROJ_MAX_COLS + 1) != -22) return 2;
  if (call(nullptr, 1) != -22) return 3;
  strom_proj_col x = c;
  x.kind = 0;
  if (call(&x, 1) != -22) return 4;
  x.kind = 5;
  if (call(&x, 1) != -22) return 5;
  x = c;
  x.width = 3;
  if (call(&x, 1) != -22) return 6;
  x = c;
  x.kind = STROM_PROJ_STR32;   // no character output
  if (call(&x, 1) != -22) return 7;
  x.out_chars = (uint64_t)(uintptr_t)chars;
  x.char_cursor = (uint64_t)(uintptr_t)&cur;
  strom_proj_col two[2] = {x, x};   // one cursor for two columns
  if (call(two, 2) != -22) return 8;
  if (total != 0) return 9;
  if (call(&c, 1) != 0 || total != 1 || out[0] != 0) return 10;
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  const uint64_t iters = argc > 1 ? strtoull(argv[1], nullptr, 0) : 1000;
  const uint64_t seed = argc > 2 ? strtoull(argv[2], nullptr, 0) : 1;
  if (int rc = bad_args()) {
    fprintf(stderr, "argument checks: case %d\n", rc);
    return 1;
  }
  for (uint64_t it = 0; it < iters; ++it) {
    rng.seed(seed * 1000003 + it);
    if (one(it)) {
      fprintf(stderr, "seed %llu\n", (unsigned long long)seed);
      return 1;
    }
  }
  printf("colproject_fuzz: %llu iterations ok (seed %llu)\n", (unsigned long long)iters,
         (unsigned long long)seed);
  return 0;
}
