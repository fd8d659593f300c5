// Randomized test of the top-k kernels' phases (csrc/kernels/coltopk.hip,
// host copy strom_topk_host_select / strom_topk_host_merge: the same append,
// bitonic sort, cut and threshold code the GPU kernels run), built host-only
// with ASan + UBSan (make build/coltopk_fuzz).  Random record batches,
// validity and selection bitmaps of every storage type go through several
// select + merge rounds against one state; the state's rows, payloads and
// counters must equal a plain std::sort of the selected rows by (class, value,
// row), compared with the type's own operators.  Every array has exactly the
// size the contract names, so a read or write past one is an ASan report.
//
//   coltopk_fuzz ITERATIONS [SEED]
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <type_traits>
#include <vector>

#include "strom/strom.h"

namespace {

struct Rec {
  int cls;           // 0 value, 1 NaN, 2 null
  int64_t i;         // the value of a signed type
  uint64_t u;        // ... of an unsigned one
  double d;          // ... of a float
  uint64_t row, pay;
  int pvalid;
};

template <typename T> T random_value(std::mt19937_64 &rng, int shape) {
  const uint64_t r = rng();
  if constexpr (std::is_floating_point<T>::value) {
    switch (r % (shape ? 4 : 12)) {
      case 0: return (T)0.0;
      case 1: return (T)-0.0;
      case 2: return (T)NAN;
      case 3: return r & 16 ? (T)INFINITY : (T)-INFINITY;
      default: return (T)((double)(int64_t)(rng() % 2001) - 1000.0) / (T)(1 + r % 7);
    }
  } else {
    typedef std::numeric_limits<T> L;
    switch (r % (shape ? 3 : 8)) {
      case 0: return L::max();
      case 1: return L::min();
      case 2: return (T)(r >> 8 & 3);
      default: return (T)rng();
    }
  }
}

template <typename T> bool value_less(const Rec &a, const Rec &b, bool desc) {
  if constexpr (std::is_floating_point<T>::value) return desc ? a.d > b.d : a.d < b.d;
  else if constexpr (std::is_signed<T>::value) return desc ? a.i > b.i : a.i < b.i;
  else return desc ? a.u > b.u : a.u < b.u;
}

template <typename T> int run_case(std::mt19937_64 &rng, int type, long *rows_checked) {
  static const uint32_t ks[] = {1, 2, 3, 7, 64, 65, 300, 1024, STROM_TOPK_MAX_K};
  static const uint32_t sizes[] = {0, 1, 63, 64, 65, 200};
  const uint32_t k = ks[rng() % 9];
  const bool desc = rng() & 1;
  const int shape = (int)(rng() % 3);          // 0 spread, 1 few distinct values, 2 sorted
  static const uint32_t widths[] = {0, 1, 2, 4, 8};
  const uint32_t pw = widths[rng() % 5];
  std::vector<uint64_t> state(strom_topk_state_words(k));
  if (strom_topk_host_init(state.data(), k)) return 1;
  std::vector<Rec> all;
  uint64_t row_base = rng() % 1000, selected = 0;
  const int rounds = 1 + (int)(rng() % 3);
  for (int round = 0; round < rounds; ++round) {
    const uint32_t nb = 1 + (uint32_t)(rng() % 5);
    std::vector<std::vector<T>> vals(nb);
    std::vector<std::vector<uint8_t>> pays(nb);
    std::vector<std::vector<uint64_t>> valid(nb), pvalid(nb);
    std::vector<strom_filter_batch> vt(nb), pt(nb);
    uint64_t nwords = 0;
    for (uint32_t b = 0; b < nb; ++b) {
      const uint32_t n = rng() % 4 ? sizes[rng() % 6] : (uint32_t)(rng() % 3000);
      const uint64_t nw = (n + 63) / 64;
      vals[b].resize(n);
      for (auto &x : vals[b]) x = random_value<T>(rng, shape);
      if (shape == 2)
        std::sort(vals[b].begin(), vals[b].end(), [&](T x, T y) {
          return x == x && y == y ? ((round & 1) ? x > y : x < y) : x == x;
        });
      pays[b].resize((size_t)n * pw);
      for (auto &x : pays[b]) x = (uint8_t)rng();
      const bool nulls = rng() & 1, pnulls = rng() & 1;
      if (nulls) {
        valid[b].resize(nw);
        for (auto &x : valid[b]) x = rng() | rng();
      }
      if (pnulls && pw) {
        pvalid[b].resize(nw);
        for (auto &x : pvalid[b]) x = rng();
      }
      vt[b] = strom_filter_batch{(uint64_t)(uintptr_t)vals[b].data(),
                                 nulls && nw ? (uint64_t)(uintptr_t)valid[b].data() : 0, n, nwords,
                                 row_base};
      pt[b] = strom_filter_batch{(uint64_t)(uintptr_t)pays[b].data(),
                                 pnulls && pw && nw ? (uint64_t)(uintptr_t)pvalid[b].data() : 0, n,
                                 nwords, row_base};
      row_base += n + rng() % 3;
      nwords += nw;
    }
    // the selection: garbage beyond each batch's rows included
    std::vector<uint64_t> bitmap(nwords);
    const int density = (int)(rng() % 4);
    for (auto &x : bitmap)
      x = density == 0 ? ~0ull : density == 1 ? rng() : density == 2 ? rng() & rng() & rng() : 0;
    for (uint32_t b = 0; b < nb; ++b)
      for (uint64_t r = 0; r < vt[b].nrows; ++r) {
        const uint64_t w = vt[b].word_base + r / 64;
        if (!((bitmap[w] >> (r % 64)) & 1)) continue;
        ++selected;
        Rec rec{};
        const T x = vals[b][r];
        rec.row = vt[b].row_base + r;
        if (vt[b].valid && !((valid[b][r / 64] >> (r % 64)) & 1)) rec.cls = 2;
        else if (x != x) rec.cls = 1;
        else {
          if constexpr (std::is_floating_point<T>::value) rec.d = (double)x;
          else if constexpr (std::is_signed<T>::value) rec.i = (int64_t)x;
          else rec.u = (uint64_t)x;
        }
        if (pw && !(pt[b].valid && !((pvalid[b][r / 64] >> (r % 64)) & 1))) {
          rec.pvalid = 1;
          memcpy(&rec.pay, pays[b].data() + r * pw, pw);
        }
        all.push_back(rec);
      }
    if (!nwords) continue;                     // nothing to launch
    const uint32_t grid = strom_column_topk_grid(nwords, k);
    std::vector<uint64_t> slabs(grid * strom_topk_slab_words(k), 0x5a5a5a5a5a5a5a5aull);
    // a select may have read the threshold before an earlier merge stored it
    std::vector<uint64_t> stale(state.begin(), state.begin() + STROM_TOPK_HDR_WORDS);
    if (rng() % 3 == 0) stale[STROM_TOPK_H_THRESH] = ~0ull;
    int rc = strom_topk_host_select(type, desc ? STROM_TOPK_DESC : 0, k, bitmap.data(), nwords,
                                    vt.data(), pw ? pt.data() : nullptr, pw, nb, stale.data(),
                                    slabs.data());
    if (rc) {
      fprintf(stderr, "select: rc %d\n", rc);
      return 1;
    }
    rc = strom_topk_host_merge(k, slabs.data(), grid, state.data());
    if (rc) {
      fprintf(stderr, "merge: rc %d\n", rc);
      return 1;
    }
  }
  std::sort(all.begin(), all.end(), [&](const Rec &a, const Rec &b) {
    if (a.cls != b.cls) return a.cls < b.cls;
    if (a.cls == 0) {
      if (value_less<T>(a, b, desc)) return true;
      if (value_less<T>(b, a, desc)) return false;
    }
    return a.row < b.row;
  });
  const uint64_t want = all.size() < k ? all.size() : k;
  if (state[STROM_TOPK_H_K] != k || state[STROM_TOPK_H_COUNT] != want ||
      state[STROM_TOPK_H_SEEN] != selected || state[STROM_TOPK_H_ERRORS] != 0) {
    fprintf(stderr, "type %d k %u: header count %llu seen %llu errors %llu, want %llu %llu 0\n",
            type, k, (unsigned long long)state[STROM_TOPK_H_COUNT],
            (unsigned long long)state[STROM_TOPK_H_SEEN],
            (unsigned long long)state[STROM_TOPK_H_ERRORS], (unsigned long long)want,
            (unsigned long long)selected);
    return 1;
  }
  for (uint64_t i = 0; i < want; ++i) {
    const uint64_t *e = &state[STROM_TOPK_HDR_WORDS + STROM_TOPK_ENTRY_WORDS * i];
    const uint64_t row = e[1] >> 2 & ((1ull << 60) - 1);
    if (row != all[i].row || (int)(e[1] >> 62) != all[i].cls || (int)(e[1] & 1) != all[i].pvalid ||
        e[2] != all[i].pay) {
      fprintf(stderr, "type %d k %u desc %d: candidate %llu is row %llu class %d, want row %llu "
              "class %d\n", type, k, (int)desc, (unsigned long long)i, (unsigned long long)row,
              (int)(e[1] >> 62), (unsigned long long)all[i].row, all[i].cls);
      return 1;
    }
  }
  *rows_checked += (long)want;
  return 0;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s ITERATIONS [SEED]\n", argv[0]);
    return 2;
  }
  const int iters = atoi(argv[1]);
  std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 1234);
  long rows = 0;
  for (int i = 0; i < iters; ++i) {
    int rc;
    switch (i % 10) {
      case 0: rc = run_case<int8_t>(rng, STROM_COL_I8, &rows); break;
      case 1: rc = run_case<int16_t>(rng, STROM_COL_I16, &rows); break;
      case 2: rc = run_case<int32_t>(rng, STROM_COL_I32, &rows); break;
      case 3: rc = run_case<int64_t>(rng, STROM_COL_I64, &rows); break;
      case 4: rc = run_case<uint8_t>(rng, STROM_COL_U8, &rows); break;
      case 5: rc = run_case<uint16_t>(rng, STROM_COL_U16, &rows); break;
      case 6: rc = run_case<uint32_t>(rng, STROM_COL_U32, &rows); break;
      case 7: rc = run_case<uint64_t>(rng, STROM_COL_U64, &rows); break;
      case 8: rc = run_case<float>(rng, STROM_COL_F32, &rows); break;
      default: rc = run_case<double>(rng, STROM_COL_F64, &rows); break;
    }
    if (rc) {
      fprintf(stderr, "iteration %d failed\n", i);
      return 1;
    }
  }
  // a malformed slab and a state of another k are counted, not followed
  std::vector<uint64_t> state(strom_topk_state_words(4)), slab(strom_topk_slab_words(4), 0);
  strom_topk_host_init(state.data(), 4);
  slab[0] = 5;
  if (strom_topk_host_merge(4, slab.data(), 1, state.data()) || state[STROM_TOPK_H_ERRORS] != 1 ||
      state[STROM_TOPK_H_COUNT] != 0)
    return 1;
  std::vector<uint64_t> slab2(strom_topk_slab_words(2), 0);
  if (strom_topk_host_merge(2, slab2.data(), 1, state.data()) ||
      state[STROM_TOPK_H_ERRORS] != 2)
    return 1;
  printf("coltopk_fuzz: %d cases ok, %ld result rows checked\n", iters, rows);
  return 0;
}
