// Randomized test of the LIKE kernel's row matcher (csrc/kernels/collike.hip,
// host copy strom_column_like_host: the same functions the GPU kernel runs,
// the wave's ballots as loops), built host-only with ASan + UBSan (make
// build/collike_fuzz).  Each iteration draws a pattern, builds its operands
// as strom.h lays them out, and draws record batches of rows at random
// alignments of their character buffers:
//   - valid UTF-8 on a utf8 column and any bytes on a binary one, compared
//     bit for bit with a backtracking matcher written here (a memoized
//     recursion over the pattern's tokens: no segments, no anchors);
//   - bytes that are no UTF-8 on a utf8 column and offset pairs that are
//     negative, decreasing or past the buffer: evaluated twice, the results
//     equal, the malformed rows never selected, NEGATE or not.
// Every buffer is allocated at exactly the size the contract names (the
// character buffer up to the dword that holds its last byte), so a read
// past one is an ASan report.
//
//   collike_fuzz ITERATIONS [SEED]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <random>
#include <string>
#include <vector>

#include "strom/strom.h"

namespace {

std::mt19937_64 rng;
uint32_t rnd(uint32_t n) { return n ? (uint32_t)(rng() % n) : 0; }

enum { T_LIT, T_ONE, T_ANY };   // a byte, '_', '%'
struct Tok {
  int kind;
  uint8_t byte;
};

const char *kChars[] = {"a", "b", "c", "\xc3\xa9", "\xe2\x82\xac", "\xf0\x9f\x98\x80", "\n"};
const uint8_t kBytes[] = {'a', 'b', 'c', 0x80, 0xA9, 0xBF, 0xC3, 0xE2, 0xF0, 0x00};

std::string rand_text(uint32_t nchars, bool utf8_valid) {
  std::string s;
  for (uint32_t i = 0; i < nchars; ++i) {
    if (utf8_valid) s += kChars[rnd(rnd(3) ? 3 : 7)];
    else s += (char)kBytes[rnd(rnd(3) ? 3 : 10)];
  }
  return s;
}

std::vector<Tok> rand_pattern(bool utf8_valid) {
  std::vector<Tok> t;
  const uint32_t n = rnd(4) ? rnd(7) : rnd(14);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t k = rnd(10);
    if (k < 3) t.push_back({T_ANY, 0});
    else if (k < 5) t.push_back({T_ONE, 0});
    else
      for (char c : rand_text(1 + rnd(3), utf8_valid)) t.push_back({T_LIT, (uint8_t)c});
  }
  return t;
}

// the operands of one pattern list, as strom.h lays them out
struct Operands {
  std::vector<uint32_t> consts, offs;
  bool wild = false;
};

void add_pattern(Operands &o, const std::vector<Tok> &t, uint32_t slot) {
  // segments: the runs between '%'
  std::vector<std::vector<Tok>> segs(1);
  bool any = false;
  for (const Tok &x : t) {
    if (x.kind == T_ANY) {
      segs.emplace_back();
      any = true;
    } else {
      segs.back().push_back(x);
    }
  }
  const bool head = !segs.front().empty() || !any, tail = !segs.back().empty() || !any;
  std::vector<std::vector<Tok>> keep;
  for (auto &s : segs)
    if (!s.empty()) keep.push_back(s);
  o.offs[slot] = (uint32_t)o.offs.size();
  const size_t at = o.offs.size();
  uint32_t least = 0;
  for (auto &s : keep) least += (uint32_t)s.size();
  o.offs.push_back((head ? STROM_LIKE_HEAD : 0) | (tail ? STROM_LIKE_TAIL : 0));
  o.offs.push_back(least);
  o.offs.push_back((uint32_t)keep.size());
  for (size_t j = 0; j < keep.size(); ++j) o.offs.push_back(0);
  for (size_t j = 0; j < keep.size(); ++j) {
    o.offs[at + 3 + j] = (uint32_t)o.offs.size();
    const size_t sa = o.offs.size();
    o.offs.push_back((uint32_t)keep[j].size());
    o.offs.push_back(0);
    o.offs.push_back(0);
    uint32_t skip = 0, npiece = 0;
    std::string lit;
    auto flush = [&] {
      if (lit.empty()) return;
      o.offs.push_back(skip);
      o.offs.push_back((uint32_t)o.consts.size() * 4);
      o.offs.push_back((uint32_t)lit.size());
      const size_t w0 = o.consts.size();
      o.consts.resize(w0 + (lit.size() + 3) / 4, 0);
      memcpy(o.consts.data() + w0, lit.data(), lit.size());
      ++npiece;
      skip = 0;
      lit.clear();
    };
    for (const Tok &x : keep[j]) {
      if (x.kind == T_ONE) {
        flush();
        ++skip;
        o.wild = true;
      } else {
        lit.push_back((char)x.byte);
      }
    }
    flush();
    o.offs[sa + 1] = npiece;
    o.offs[sa + 2] = skip;   // the '_' after the last piece
  }
}

// ---- the reference: memoized backtracking over the tokens
struct Ref {
  const std::vector<Tok> &t;
  const uint8_t *r;
  uint32_t len;
  bool utf8;
  std::vector<int8_t> memo;
  Ref(const std::vector<Tok> &t_, const uint8_t *r_, uint32_t len_, bool utf8_)
      : t(t_), r(r_), len(len_), utf8(utf8_), memo((t_.size() + 1) * (size_t)(len_ + 1), -1) {}
  bool go(size_t ti, uint32_t p) {
    int8_t &m = memo[ti * (len + 1) + p];
    if (m >= 0) return m;
    bool ok;
    if (ti == t.size()) {
      ok = p == len;
    } else if (t[ti].kind == T_LIT) {
      ok = p < len && r[p] == t[ti].byte && go(ti + 1, p + 1);
    } else if (t[ti].kind == T_ONE) {
      ok = false;
      if (p < len) {
        uint32_t q = p + 1;
        while (utf8 && q < len && (r[q] & 0xC0) == 0x80) ++q;
        ok = go(ti + 1, q);
      }
    } else {
      ok = false;
      for (uint32_t q = p; q <= len && !ok; ++q) ok = go(ti + 1, q);
    }
    m = ok;
    return ok;
  }
};

// ---- tables
struct Batch {
  std::vector<uint32_t> chars;     // whole dwords: up to the one holding the last byte
  uint64_t nchars = 0;
  std::vector<int32_t> o32;
  std::vector<int64_t> o64;
  std::vector<uint64_t> valid;     // empty: none
  std::vector<std::string> rows;
  std::vector<bool> bad;
};

struct Table {
  std::vector<Batch> b;
  std::vector<strom_qual_batch> qb;
  uint64_t nwords = 0;
  bool wide = false;
};

void build(Table &t, bool wide, bool utf8_valid, bool malformed) {
  t.wide = wide;
  const uint32_t nb = 1 + rnd(3);
  t.b.resize(nb);
  for (auto &b : t.b) {
    const uint32_t n = rnd(5) ? rnd(150) : 0;
    std::string chars;
    std::vector<int64_t> offs{0};
    for (uint32_t i = 0; i < n; ++i) {
      uint32_t nch = rnd(4) ? rnd(12) : rnd(40);
      if (!rnd(40)) nch = 200 + rnd(400);          // past STROM_LIKE_LONG_ROW
      std::string r = rand_text(nch, utf8_valid);
      if (!rnd(3)) {                               // a gap: the next row at another alignment
        chars += std::string(1 + rnd(3), utf8_valid ? 'z' : (char)(0x80 + rnd(0x40)));
        offs.back() = (int64_t)chars.size();
      }
      chars += r;
      offs.push_back((int64_t)chars.size());
      b.rows.push_back(r);
    }
    b.bad.assign(n, false);
    if (malformed && n >= 4) {
      for (int k = 0; k < 3; ++k) {
        const uint32_t j = 1 + rnd(n - 1);         // the offset between rows j - 1 and j
        if (k == 0) offs[j] = -1 - (int64_t)rnd(100);
        else if (k == 1) offs[j] = (int64_t)chars.size() + 1 + (wide ? (int64_t)rng() % (1ll << 40) : rnd(1000));
        else offs[j] = offs[j - 1] - 1 - rnd(5);
      }
      for (uint32_t i = 0; i < n; ++i)
        b.bad[i] = offs[i] < 0 || offs[i + 1] < offs[i] || (uint64_t)offs[i + 1] > chars.size();
    }
    b.nchars = chars.size();
    b.chars.assign((chars.size() + 3) / 4, 0);
    if (!chars.empty()) memcpy(b.chars.data(), chars.data(), chars.size());
    if (b.chars.size() * 4 > chars.size())         // bytes past aux_len in the last dword: junk
      memset((uint8_t *)b.chars.data() + chars.size(), 0x61, b.chars.size() * 4 - chars.size());
    if (wide) b.o64.assign(offs.begin(), offs.end());
    else
      for (int64_t x : offs) b.o32.push_back((int32_t)x);
    if (n && rnd(2)) {
      b.valid.resize((n + 63) / 64);
      for (auto &w : b.valid) w = rng() | rng();   // 3/4 valid, bits past nrows dirty
    }
    // rows kept as the offsets now say (a malformed neighbour changes a row's span)
    for (uint32_t i = 0; i < n; ++i)
      if (!b.bad[i]) b.rows[i] = chars.substr((size_t)offs[i], (size_t)(offs[i + 1] - offs[i]));
  }
  uint64_t w = 0, row = 0;
  for (auto &b : t.b) {
    strom_qual_batch q{};
    q.values = wide ? (uint64_t)(uintptr_t)b.o64.data() : (uint64_t)(uintptr_t)b.o32.data();
    q.valid = b.valid.empty() ? 0 : (uint64_t)(uintptr_t)b.valid.data();
    q.nrows = b.rows.size();
    q.word_base = w;
    q.row_base = row;
    q.aux = (uint64_t)(uintptr_t)b.chars.data();
    q.aux_len = b.nchars;
    t.qb.push_back(q);
    w += (b.rows.size() + 63) / 64;
    row += b.rows.size();
  }
  t.nwords = w;
}

int fail(const char *what, uint64_t it, uint64_t w) {
  printf("FAIL %s: case %llu word %llu\n", what, (unsigned long long)it, (unsigned long long)w);
  return 1;
}

}  // namespace

int main(int argc, char **argv) {
  const uint64_t iters = argc > 1 ? strtoull(argv[1], nullptr, 10) : 400;
  rng.seed(argc > 2 ? strtoull(argv[2], nullptr, 10) : 12345);
  uint64_t selected = 0, longrows = 0;
  for (uint64_t it = 0; it < iters; ++it) {
    const bool utf8 = rnd(2), wide = rnd(2);
    const bool malformed = it % 3 == 2;            // junk bytes + malformed offsets
    const bool valid_text = utf8 && !malformed;
    const uint32_t npat = 1 + (rnd(4) ? 0 : rnd(3));
    std::vector<std::vector<Tok>> pats;
    Operands o;
    o.offs.assign(npat, 0);
    for (uint32_t k = 0; k < npat; ++k) {
      pats.push_back(rand_pattern(utf8));
      add_pattern(o, pats.back(), k);
    }
    if (o.consts.empty()) o.consts.push_back(0);
    Table t;
    build(t, wide, valid_text, malformed);
    strom_col_qual q{};
    q.type = wide ? STROM_COL_STR64 : STROM_COL_STR32;
    q.op = STROM_QOP_STR_LIKE;
    const bool neg = rnd(2);
    q.flags = (neg ? STROM_QUAL_NEGATE : 0) | (o.wild ? STROM_QUAL_LIKE_WILD : 0) |
              (o.wild && utf8 ? STROM_QUAL_LIKE_UTF8 : 0);
    q.nconst = npat;
    q.consts = (uint64_t)(uintptr_t)o.consts.data();
    q.offs = (uint64_t)(uintptr_t)o.offs.data();
    q.const_bytes = o.consts.size() * 4;
    q.offs_bytes = o.offs.size() * 4;
    const bool use_or = rnd(2), and_dst = rnd(2);
    std::vector<uint64_t> old(t.nwords + 1), orw(t.nwords + 1), bm, bm2;
    for (auto &x : old) x = rng();
    for (auto &x : orw) x = rng() & rng();
    bm = old;
    uint64_t cnt = 5, cnt2 = 5;
    int rc = strom_column_like_host(&q, t.qb.data(), (uint32_t)t.qb.size(), t.nwords, bm.data(),
                                    use_or ? orw.data() : nullptr, and_dst, &cnt);
    if (rc != 0) return fail("rc", it, (uint64_t)rc);
    bm2 = old;
    rc = strom_column_like_host(&q, t.qb.data(), (uint32_t)t.qb.size(), t.nwords, bm2.data(),
                                use_or ? orw.data() : nullptr, and_dst, &cnt2);
    if (rc != 0 || bm2 != bm || cnt2 != cnt) return fail("second evaluation differs", it, 0);
    if (t.nwords && bm[t.nwords] != old[t.nwords]) return fail("guard word", it, t.nwords);
    // expected words
    uint64_t total = 5;
    for (size_t k = 0; k < t.b.size(); ++k) {
      const Batch &b = t.b[k];
      for (uint64_t i0 = 0; i0 < b.rows.size(); i0 += 64) {
        const uint64_t w = t.qb[k].word_base + i0 / 64;
        uint64_t pred = 0, known = 0;
        for (uint64_t i = i0; i < b.rows.size() && i < i0 + 64; ++i) {
          const bool ok = b.valid.empty() || ((b.valid[i / 64] >> (i % 64)) & 1);
          known |= 1ull << (i - i0);
          if (!ok || b.bad[i]) continue;             // selected by no form
          if (malformed && utf8) {                   // no reference: the bit is the host copy's
            known &= ~(1ull << (i - i0));
            continue;
          }
          const std::string &r = b.rows[i];
          bool h = false;
          for (auto &p : pats) {
            Ref ref(p, (const uint8_t *)r.data(), (uint32_t)r.size(), utf8);
            h = h || ref.go(0, 0);
          }
          if (h != neg) pred |= 1ull << (i - i0);
          if (r.size() > STROM_LIKE_LONG_ROW) ++longrows;
        }
        // bits of rows past nrows are clear; unknown bits are taken from the result
        uint64_t got = bm[w];
        uint64_t exp = pred;
        if (use_or) exp |= orw[w];
        if (and_dst) exp &= old[w];
        const uint64_t care = known | ~((b.rows.size() - i0 >= 64) ? ~0ull : ((1ull << (b.rows.size() - i0)) - 1));
        uint64_t decided = care;
        if (use_or) decided |= orw[w];               // an OR-ed 1 decides the bit whatever the row
        if (and_dst) decided |= ~old[w];             // an AND-ed 0 too
        if ((got ^ exp) & decided) return fail("bits", it, w);
        total += (uint64_t)__builtin_popcountll(got);
        selected += (uint64_t)__builtin_popcountll(pred);
      }
    }
    if (cnt != total) return fail("count", it, cnt);
  }
  if (!selected || !longrows) {
    printf("FAIL: nothing selected (%llu) or no long row (%llu)\n", (unsigned long long)selected,
           (unsigned long long)longrows);
    return 1;
  }
  // operands the check refuses: a record or a piece outside its blob
  {
    Operands o;
    o.offs.assign(1, 0);
    add_pattern(o, {{T_LIT, 'a'}, {T_ONE, 0}, {T_LIT, 'b'}}, 0);
    Table t;
    while (!t.nwords) {
      t = Table();
      build(t, false, true, false);
    }
    strom_col_qual q{};
    q.type = STROM_COL_STR32;
    q.op = STROM_QOP_STR_LIKE;
    q.flags = STROM_QUAL_LIKE_WILD;
    q.nconst = 1;
    q.consts = (uint64_t)(uintptr_t)o.consts.data();
    q.const_bytes = o.consts.size() * 4;
    std::vector<uint64_t> bm(t.nwords + 1, 7);
    uint64_t cnt = 0;
    for (size_t at = 0; at < o.offs.size(); ++at) {
      std::vector<uint32_t> x = o.offs;
      x[at] = 0x7fffffffu;
      q.offs = (uint64_t)(uintptr_t)x.data();
      q.offs_bytes = x.size() * 4;
      const int rc = strom_column_like_host(&q, t.qb.data(), (uint32_t)t.qb.size(), t.nwords,
                                            bm.data(), nullptr, 0, &cnt);
      // the flags, the least-bytes words and a '_' count only change the answer
      const bool harmless = at == 1 || at == 2 || at == 5 || at == 7 || at == 8 || at == 11;
      if (rc != (harmless ? 0 : -22)) return fail("operand check", at, (uint64_t)rc);
    }
  }
  printf("%llu cases ok (%llu rows selected, %llu long rows)\n", (unsigned long long)iters,
         (unsigned long long)selected, (unsigned long long)longrows);
  return 0;
}
