// Randomized test of the computed-column kernel's walk (csrc/kernels/colexpr.hip,
// host copy strom_column_expr_host: the same loads, ops and validity words
// the GPU kernel runs), built host-only with ASan + UBSan (make
// build/colexpr_fuzz).  Each iteration builds a random valid program over
// random record batches of random source types, validity and selection words
// and compares every output word with a plain scalar evaluation written here
// (128-bit integers for the floor division, one double operation per op);
// then it breaks the program in one of the ways strom_expr_check names and
// requires -22 from the check and from the walk, with the output untouched.
// Every array has exactly the size the contract names, so a read or write
// past one is an ASan report.
//
//   colexpr_fuzz ITERATIONS [SEED]
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <vector>

#include "strom/strom.h"

#pragma clang fp contract(off)

namespace {

constexpr uint64_t kPrefill = 0xA5A5A5A5A5A5A5A5ull;
constexpr uint64_t kNaN = 0x7ff8000000000000ull;
const uint32_t kIntTypes[] = {STROM_COL_I8,  STROM_COL_I16, STROM_COL_I32, STROM_COL_I64,
                              STROM_COL_U8,  STROM_COL_U16, STROM_COL_U32};
const uint32_t kFltTypes[] = {STROM_COL_F32, STROM_COL_F64};

uint32_t width_of(uint32_t t) {
  switch (t) {
    case STROM_COL_I8: case STROM_COL_U8: return 1;
    case STROM_COL_I16: case STROM_COL_U16: return 2;
    case STROM_COL_I32: case STROM_COL_U32: case STROM_COL_F32: return 4;
    default: return 8;
  }
}

double f_of(uint64_t x) {
  double d;
  memcpy(&d, &x, 8);
  return d;
}

uint64_t u_of(double d) {
  uint64_t x;
  memcpy(&x, &d, 8);
  return x;
}

// one source value, widened as strom.h says
uint64_t ref_load(uint32_t type, const uint8_t *p, uint64_t i, bool flt) {
  int64_t v = 0;
  switch (type) {
    case STROM_COL_I8: { int8_t x; memcpy(&x, p + i, 1); v = x; break; }
    case STROM_COL_I16: { int16_t x; memcpy(&x, p + 2 * i, 2); v = x; break; }
    case STROM_COL_I32: { int32_t x; memcpy(&x, p + 4 * i, 4); v = x; break; }
    case STROM_COL_I64: { int64_t x; memcpy(&x, p + 8 * i, 8); v = x; break; }
    case STROM_COL_U8: { uint8_t x; memcpy(&x, p + i, 1); v = x; break; }
    case STROM_COL_U16: { uint16_t x; memcpy(&x, p + 2 * i, 2); v = x; break; }
    case STROM_COL_U32: { uint32_t x; memcpy(&x, p + 4 * i, 4); v = x; break; }
    case STROM_COL_F32: { float x; memcpy(&x, p + 4 * i, 4); return u_of((double)x); }
    default: { uint64_t x; memcpy(&x, p + 8 * i, 8); return x; }
  }
  return flt ? u_of((double)v) : (uint64_t)v;
}

struct Table {
  uint32_t ncols = 0;
  std::vector<uint64_t> rows;                          // per batch
  std::vector<std::vector<std::vector<uint8_t>>> vals; // [col][batch] bytes
  std::vector<std::vector<std::vector<uint64_t>>> ok;  // [col][batch] words (empty: none)
  std::vector<std::vector<uint64_t>> out_vals, out_ok; // [batch]
  std::vector<strom_filter_batch> src, out;            // src: ncols tables of nbatches
  uint64_t nwords = 0;
};

uint64_t random_bits(std::mt19937_64 &rng, uint32_t type) {
  const uint64_t r = rng();
  if (type == STROM_COL_F32 || type == STROM_COL_F64) {
    double d;
    switch (r % 16) {
      case 0: d = 0.0; break;
      case 1: d = -0.0; break;
      case 2: d = NAN; break;
      case 3: d = r & 64 ? INFINITY : -INFINITY; break;
      case 4: d = 4.9e-324 * (double)(r >> 60); break;
      case 5: d = 1e300; break;
      default: d = ((double)(int64_t)(rng() % 200001) - 100000.0) / (double)(1 + (r >> 8) % 9);
    }
    if (type == STROM_COL_F32) {
      if (d == 1e300) d = 1e30;
      const float f = (float)d;
      uint32_t w;
      memcpy(&w, &f, 4);
      return w;
    }
    return u_of(d);
  }
  switch (r % 8) {
    case 0: return ~0ull >> 1;         // the type's bytes of INT64_MAX
    case 1: return 1ull << 63;         // ... of INT64_MIN (0 for narrower types)
    case 2: return ~0ull;
    case 3: return (r >> 8) & 7;
    case 4: return 1ull << (8 * width_of(type) - 1);
    default: return rng();
  }
}

void build_table(std::mt19937_64 &rng, Table &t, const strom_expr &e) {
  const uint32_t nb = 1 + rng() % 5;
  t.ncols = e.ncols;
  t.rows.resize(nb);
  uint64_t wb = 0;
  std::vector<uint64_t> base(nb);
  for (uint32_t b = 0; b < nb; ++b) {
    static const uint64_t shapes[] = {1, 63, 64, 65, 127, 128, 200};
    t.rows[b] = rng() % 4 ? shapes[rng() % 7] : rng() % 260;
    if (b + 1 == nb && t.rows[b] == 0) t.rows[b] = 1;
    base[b] = wb;
    wb += (t.rows[b] + 63) / 64;
  }
  t.nwords = wb;
  t.vals.assign(t.ncols, {});
  t.ok.assign(t.ncols, {});
  t.src.assign((size_t)t.ncols * nb, strom_filter_batch{});
  for (uint32_t c = 0; c < t.ncols; ++c) {
    const uint32_t w = width_of(e.col_type[c]);
    const int nulls = rng() % 3;       // 0 none, 1 every batch, 2 some batches
    t.vals[c].resize(nb);
    t.ok[c].resize(nb);
    for (uint32_t b = 0; b < nb; ++b) {
      t.vals[c][b].resize(t.rows[b] * w);
      for (uint64_t i = 0; i < t.rows[b]; ++i) {
        const uint64_t x = random_bits(rng, e.col_type[c]);
        memcpy(t.vals[c][b].data() + i * w, &x, w);
      }
      if (nulls == 1 || (nulls == 2 && rng() % 2)) {
        t.ok[c][b].resize((t.rows[b] + 63) / 64);
        // bits past nrows are set too: the walk must cut them
        for (auto &x : t.ok[c][b]) x = rng() % 5 ? (rng() | rng()) : (rng() % 2 ? 0 : ~0ull);
      }
      strom_filter_batch &s = t.src[(size_t)c * nb + b];
      s.values = (uint64_t)(uintptr_t)t.vals[c][b].data();
      s.valid = t.ok[c][b].empty() ? 0 : (uint64_t)(uintptr_t)t.ok[c][b].data();
      s.nrows = t.rows[b];
      s.word_base = base[b];
    }
  }
  t.out_vals.resize(nb);
  t.out_ok.resize(nb);
  t.out.assign(nb, strom_filter_batch{});
  for (uint32_t b = 0; b < nb; ++b) {
    t.out_vals[b].assign(t.rows[b], kPrefill);
    t.out_ok[b].assign((t.rows[b] + 63) / 64, kPrefill);
    t.out[b].values = (uint64_t)(uintptr_t)t.out_vals[b].data();
    t.out[b].valid = (uint64_t)(uintptr_t)t.out_ok[b].data();
    t.out[b].nrows = t.rows[b];
    t.out[b].word_base = base[b];
  }
}

// a random program that strom_expr_check accepts
void build_program(std::mt19937_64 &rng, strom_expr &e) {
  memset(&e, 0, sizeof(e));
  const bool flt = rng() % 2;
  e.domain = flt ? STROM_EXPR_FLT : STROM_EXPR_INT;
  e.ncols = 1 + rng() % STROM_EXPR_MAX_COLS;
  for (uint32_t c = 0; c < e.ncols; ++c)
    e.col_type[c] = flt && rng() % 2 ? kFltTypes[rng() % 2] : kIntTypes[rng() % 7];
  const uint32_t n = 1 + rng() % STROM_EXPR_MAX_OPS;
  uint32_t depth = 0;
  for (uint32_t p = 0; p < n; ++p) {
    const uint32_t left = n - p;       // ops still to place, this one included
    // after this op, depth - 1 binary ops must still fit
    const bool can_push = depth < STROM_EXPR_MAX_DEPTH && depth + 1 - 1 <= left - 1;
    const bool can_un = depth >= 1 && depth - 1 <= left - 1;
    const bool can_bin = depth >= 2;
    const bool must_bin = depth >= 1 && depth - 1 == left;   // only binaries reach depth 1
    strom_expr_op &o = e.ops[p];
    int kind;
    if (depth == 0) kind = 0;
    else if (must_bin) kind = 2;
    else {
      do kind = rng() % 3;
      while ((kind == 0 && !can_push) || (kind == 1 && !can_un) || (kind == 2 && !can_bin));
    }
    if (kind == 0) {
      if (rng() % 3) {
        o.op = STROM_XOP_COL;
        o.arg = rng() % e.ncols;
      } else {
        o.op = STROM_XOP_CONST;
        o.imm = flt ? random_bits(rng, STROM_COL_F64)
                    : (rng() % 2 ? (uint64_t)(int64_t)((int)(rng() % 41) - 20) : rng());
      }
      ++depth;
    } else if (kind == 1) {
      const uint32_t pick = rng() % (flt ? 2 : 4);
      o.op = pick == 0 ? STROM_XOP_NEG : pick == 1 ? STROM_XOP_ABS
             : pick == 2 ? STROM_XOP_FDIV : STROM_XOP_MOD;
      if (pick >= 2) {
        static const uint64_t divs[] = {1, 2, 7, 1000, 1ull << 40, ~0ull >> 1};
        o.imm = divs[rng() % 6];
      }
    } else {
      const uint32_t pick = rng() % (flt ? 4 : 3);
      o.op = pick == 0 ? STROM_XOP_ADD : pick == 1 ? STROM_XOP_SUB
             : pick == 2 ? STROM_XOP_MUL : STROM_XOP_DIV;
      --depth;
    }
  }
  e.nops = n;
}

uint64_t ref_eval(const strom_expr &e, const Table &t, uint32_t nb, uint32_t b, uint64_t i) {
  const bool flt = e.domain == STROM_EXPR_FLT;
  uint64_t s[STROM_EXPR_MAX_DEPTH];
  uint32_t d = 0;
  for (uint32_t p = 0; p < e.nops; ++p) {
    const strom_expr_op &o = e.ops[p];
    switch (o.op) {
      case STROM_XOP_COL:
        s[d++] = ref_load(e.col_type[o.arg], t.vals[o.arg][b].data(), i, flt);
        break;
      case STROM_XOP_CONST: s[d++] = o.imm; break;
      case STROM_XOP_NEG:
        s[d - 1] = flt ? s[d - 1] ^ (1ull << 63) : (uint64_t)(-(__int128)(int64_t)s[d - 1]);
        break;
      case STROM_XOP_ABS:
        if (flt) s[d - 1] &= ~(1ull << 63);
        else {
          const __int128 x = (int64_t)s[d - 1];
          s[d - 1] = (uint64_t)(x < 0 ? -x : x);
        }
        break;
      case STROM_XOP_FDIV:
      case STROM_XOP_MOD: {
        const __int128 x = (int64_t)s[d - 1], c = (int64_t)o.imm;
        __int128 q = x / c;
        if (x % c != 0 && x < 0) --q;
        s[d - 1] = (uint64_t)(o.op == STROM_XOP_FDIV ? q : x - q * c);
        break;
      }
      default: {
        const uint64_t a = s[d - 2], bb = s[d - 1];
        --d;
        if (flt) {
          volatile double x = f_of(a), y = f_of(bb), r;
          r = o.op == STROM_XOP_ADD ? x + y : o.op == STROM_XOP_SUB ? x - y
              : o.op == STROM_XOP_MUL ? x * y : x / y;
          s[d - 1] = u_of(r);
        } else {
          const unsigned __int128 x = a, y = bb;
          s[d - 1] = (uint64_t)(o.op == STROM_XOP_ADD ? x + y : o.op == STROM_XOP_SUB ? x - y
                                                                                      : x * y);
        }
      }
    }
  }
  if (flt && f_of(s[0]) != f_of(s[0])) return kNaN;
  return s[0];
}

int check_untouched(const Table &t, const char *what) {
  for (size_t b = 0; b < t.out.size(); ++b) {
    for (uint64_t x : t.out_vals[b])
      if (x != kPrefill) return fprintf(stderr, "%s: a value was written\n", what), 1;
    for (uint64_t x : t.out_ok[b])
      if (x != kPrefill) return fprintf(stderr, "%s: a validity word was written\n", what), 1;
  }
  return 0;
}

int run_valid(std::mt19937_64 &rng, const strom_expr &e, Table &t, long *rows) {
  const uint32_t nb = (uint32_t)t.rows.size();
  if (strom_expr_check(&e) != 0) return fprintf(stderr, "a valid program was refused\n"), 1;
  std::vector<uint64_t> sel;
  const int sk = rng() % 4;            // 0 NULL, 1 ones, 2 sparse, 3 with zero words
  if (sk) {
    sel.resize(t.nwords);
    for (auto &w : sel) w = sk == 1 ? ~0ull : sk == 2 ? (rng() & rng() & rng()) | 1
                                                     : (rng() % 2 ? 0 : rng() | 1);
  }
  const int rc = strom_column_expr_host(&e, t.src.data(), nb, t.nwords,
                                        sk ? sel.data() : nullptr, t.out.data());
  if (rc) return fprintf(stderr, "host walk rc %d\n", rc), 1;
  for (uint32_t b = 0; b < nb; ++b) {
    for (uint64_t k = 0; k * 64 < t.rows[b]; ++k) {
      const uint64_t left = t.rows[b] - k * 64;
      uint64_t want = left >= 64 ? ~0ull : (1ull << left) - 1;
      for (uint32_t c = 0; c < e.ncols; ++c)
        if (!t.ok[c][b].empty()) want &= t.ok[c][b][k];
      if (sk && sel[t.out[b].word_base + k] == 0) want = 0;
      if (t.out_ok[b][k] != want)
        return fprintf(stderr, "batch %u word %llu: validity %llx, expected %llx\n", b,
                       (unsigned long long)k, (unsigned long long)t.out_ok[b][k],
                       (unsigned long long)want), 1;
      for (uint32_t l = 0; l < 64 && k * 64 + l < t.rows[b]; ++l) {
        const uint64_t i = k * 64 + l;
        const uint64_t exp = (want >> l) & 1 ? ref_eval(e, t, nb, b, i) : kPrefill;
        if (t.out_vals[b][i] != exp)
          return fprintf(stderr, "batch %u row %llu: %llx, expected %llx\n", b,
                         (unsigned long long)i, (unsigned long long)t.out_vals[b][i],
                         (unsigned long long)exp), 1;
        ++*rows;
      }
    }
  }
  return 0;
}

// one of the ways a program is malformed
const char *break_program(std::mt19937_64 &rng, strom_expr &e) {
  const bool flt = e.domain == STROM_EXPR_FLT;
  switch (rng() % 14) {
    case 0: e.ops[rng() % e.nops].op = 0; return "opcode 0";
    case 1: e.ops[rng() % e.nops].op = STROM_XOP_MOD + 1 + rng() % 1000; return "unknown opcode";
    case 2: e.nops = 0; return "no ops";
    case 3: e.nops = STROM_EXPR_MAX_OPS + 1 + rng() % 100; return "too many ops";
    case 4: e.ncols = STROM_EXPR_MAX_COLS + 1 + rng() % 100; return "too many columns";
    case 5: {
      static const uint32_t bad[] = {0, STROM_COL_U64, STROM_COL_BOOL, STROM_COL_STR32,
                                     STROM_COL_DEC128, 99};
      e.col_type[rng() % e.ncols] = bad[rng() % 6];
      return "source type";
    }
    case 6:
      if (flt) { e.domain = 2 + rng() % 100; return "domain"; }
      e.col_type[rng() % e.ncols] = kFltTypes[rng() % 2];
      return "float source in the int domain";
    case 7:
      e.ops[0].op = STROM_XOP_COL;
      e.ops[0].arg = e.ncols + rng() % 100;
      return "column index";
    case 8: e.ops[0].op = rng() % 2 ? STROM_XOP_ADD : STROM_XOP_NEG; return "underflow";
    case 9:
      for (uint32_t p = 0; p < STROM_EXPR_MAX_DEPTH + 1; ++p) {
        e.ops[p].op = STROM_XOP_CONST;
        e.ops[p].imm = 1;
      }
      for (uint32_t p = STROM_EXPR_MAX_DEPTH + 1; p < STROM_EXPR_MAX_OPS; ++p)
        e.ops[p].op = flt ? STROM_XOP_SUB : STROM_XOP_MUL;
      e.nops = STROM_EXPR_MAX_OPS;
      return "overflow";
    case 10:
      if (e.nops == STROM_EXPR_MAX_OPS) { e.nops = 0; return "no ops"; }
      e.ops[e.nops].op = STROM_XOP_CONST;
      e.ops[e.nops++].imm = 0;
      return "final depth 2";
    case 11:
      e.ops[0].op = STROM_XOP_CONST;
      e.ops[1].op = flt ? (rng() % 2 ? STROM_XOP_FDIV : STROM_XOP_MOD) : STROM_XOP_CONST;
      e.ops[1].imm = 3;
      e.ops[2].op = STROM_XOP_DIV;     // int: DIV; flt: FDIV / MOD before it
      e.nops = flt ? 2 : 3;
      return "an op of the other domain";
    case 12:
      if (flt) { e.nops = 0; return "no ops"; }
      e.ops[0].op = STROM_XOP_CONST;
      e.ops[1].op = rng() % 2 ? STROM_XOP_FDIV : STROM_XOP_MOD;
      e.ops[1].imm = rng() % 2 ? 0 : (uint64_t)(-(int64_t)(1 + rng() % 1000));
      e.nops = 2;
      return "divisor <= 0";
    default: e.ops[0].op = STROM_XOP_SUB; return "leading binary op";
  }
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: %s ITERATIONS [SEED]\n", argv[0]);
    return 2;
  }
  const int iters = atoi(argv[1]);
  std::mt19937_64 rng(argc > 2 ? strtoull(argv[2], nullptr, 10) : 4321);
  long rows = 0, refused = 0;
  for (int i = 0; i < iters; ++i) {
    strom_expr e;
    build_program(rng, e);
    Table t;
    build_table(rng, t, e);
    if (run_valid(rng, e, t, &rows)) {
      fprintf(stderr, "iteration %d failed (domain %u, %u ops, %u columns)\n", i, e.domain, e.nops,
              e.ncols);
      return 1;
    }
    // the same tables, output prefilled again, under a broken program
    for (size_t b = 0; b < t.out.size(); ++b) {
      t.out_vals[b].assign(t.out_vals[b].size(), kPrefill);
      t.out_ok[b].assign(t.out_ok[b].size(), kPrefill);
    }
    strom_expr bad = e;
    const char *what = break_program(rng, bad);
    if (strom_expr_check(&bad) != -22) {
      fprintf(stderr, "iteration %d: %s was accepted\n", i, what);
      return 1;
    }
    if (strom_column_expr_host(&bad, t.src.data(), (uint32_t)t.rows.size(), t.nwords, nullptr,
                               t.out.data()) != -22 || check_untouched(t, what)) {
      fprintf(stderr, "iteration %d: %s was evaluated\n", i, what);
      return 1;
    }
    ++refused;
  }
  if (strom_expr_check(nullptr) != -22) return fprintf(stderr, "NULL accepted\n"), 1;
  printf("%d cases ok (%ld rows, %ld malformed programs refused)\n", iters, rows, refused);
  return 0;
}
