// Mutation test of the heap scan's host copy (csrc/kernels/heapscan.hip,
// strom_heap_scan2_host / strom_heap_project_host: the page header checks,
// deformer, qualifier evaluators and snapshot check the GPU kernels run), built
// host-only with ASan + UBSan (make build/heapscan_fuzz).
//
// The input file (tests/test_heapcorpus_cpu.py writes it) holds the hand-built
// corpus pages and their seeded mutants, each with its tuple descriptor and
// the compiled qualifier sets of its case.  Every record is scanned as it is
// and under ROUNDS random mutations of its own, in all three evaluator modes
// (gen 0, the fixed AND list, the program), with and without a snapshot, and
// every column of the kept tuples is projected.  Pages, programs, pools and
// outputs are heap allocations of exactly the size the contract names, so a
// read or write one byte past any of them is an ASan report.  Checked: items
// ascending, line numbers within the page's line pointers, counts within the
// line pointers, status bits within the known set, valid in {0, 1, 2},
// projected varlena ranges inside their page, and the fixed list and the
// program of one qualifier set agreeing.
//
//   heapscan_fuzz FILE ROUNDS [SEED]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <random>
#include <vector>

#include "strom/strom.h"

namespace {

struct QualSet {
  uint32_t nfixed;                       // 0xFFFFFFFF: no fixed form
  strom_heap_qual fixed[STROM_HEAP_MAX_QUALS];
  uint32_t nprog, pool_len;
  std::unique_ptr<uint8_t[]> prog, pool;   // exact sizes
};

struct Record {
  uint32_t page_sz, npages, mutant;
  std::vector<uint8_t> pages;
  strom_heap_tupdesc desc;
  std::vector<QualSet> sets;
};

struct Totals {
  long accepted = 0, rejected = 0, kept = 0, dropped = 0, rechecked = 0, projected = 0;
  long mutated = 0, mutated_accepted = 0;
};

struct Reader {
  const uint8_t *p, *end;
  bool take(void *dst, size_t n) {
    if ((size_t)(end - p) < n) return false;
    memcpy(dst, p, n);
    p += n;
    return true;
  }
  bool u32(uint32_t *v) { return take(v, 4); }
};

#define FAIL(...)                    \
  do {                               \
    fprintf(stderr, __VA_ARGS__);    \
    fprintf(stderr, "\n");           \
    return 1;                        \
  } while (0)

// the snapshot of the "with a snapshot" runs: xids 100..199 in doubt, 150 and
// 160 running, a commit log for xids 0..255 (every fourth aborted)
struct Snapshot {
  strom_pg_mvcc m;
  std::unique_ptr<uint32_t[]> xip;
  std::unique_ptr<uint8_t[]> clog;
  Snapshot() : xip(new uint32_t[2]), clog(new uint8_t[64]) {
    memset(&m, 0, sizeof m);
    xip[0] = 150;
    xip[1] = 160;
    for (int i = 0; i < 64; ++i) clog[i] = 0x95;   // committed, committed, committed, aborted
    m.xmin = 100;
    m.xmax = 200;
    m.xip = xip.get();
    m.nxip = 2;
    m.curcid = 3;
    m.clog = clog.get();
    m.clog_n = 256;
  }
};

// one scan: exact-size outputs, the invariants; items out for the projection
int scan_once(const Record &r, const uint8_t *pages, int gen, const QualSet *qs, bool snap,
              const Snapshot &sn, uint32_t cap, uint32_t flags, std::vector<uint32_t> *items_out,
              std::vector<uint32_t> *status_out, uint32_t *recheck_out, Totals *t, bool count) {
  strom_heap_scan2_args g;
  memset(&g, 0, sizeof g);
  std::unique_ptr<uint32_t[]> items(new uint32_t[cap ? cap : 1]);
  std::unique_ptr<uint32_t[]> status(new uint32_t[r.npages]);
  std::unique_ptr<uint32_t[]> cnt(new uint32_t[3]);
  cnt[0] = cnt[1] = cnt[2] = 0;
  g.base.pages = pages;
  g.base.npages = r.npages;
  g.base.page_sz = r.page_sz;
  g.base.flags = flags;
  g.base.attr_off = -1;
  g.base.attr_width = 8;
  g.base.out_items = cap ? items.get() : nullptr;
  g.base.out_cap = cap;
  g.base.out_count = &cnt[0];
  g.base.page_status = status.get();
  g.recheck_count = &cnt[1];
  g.mvcc_removed = &cnt[2];
  if (gen == 0) {
    g.base.attr_off = 0;
    g.base.attr_width = 4;
    g.base.lo = 0;
    g.base.hi = 1000;
  } else {
    g.desc = r.desc;
    if (gen == 1) {
      g.nquals = (int32_t)qs->nfixed;
      memcpy(g.quals, qs->fixed, sizeof g.quals);
    } else {
      g.prog = (const strom_heap_qual2 *)qs->prog.get();
      g.cpool = qs->pool.get();
      g.nprog = qs->nprog;
      g.cpool_len = qs->pool_len;
    }
  }
  if (snap) {
    g.mvcc = sn.m;
    g.mvcc_on = 1;
  }
  const int rc = strom_heap_scan2_host(&g, gen);
  if (rc) FAIL("scan gen %d: rc %d", gen, rc);
  uint32_t nitems_all = 0;
  for (uint32_t pg = 0; pg < r.npages; ++pg) {
    if (status[pg] & ~0xFu) FAIL("page status %x", status[pg]);
    if (status[pg] & ~STROM_PAGE_RECHECK) {
      if (status[pg] & STROM_PAGE_RECHECK) FAIL("a rejected page asks for a recheck");
      if (count) ++t->rejected;
      continue;
    }
    if (count) ++t->accepted;
    const uint8_t *page = pages + (size_t)pg * r.page_sz;
    const uint32_t lower = (uint32_t)page[12] | ((uint32_t)page[13] << 8);
    nitems_all += (lower - 24) / 4;
  }
  const uint32_t total = cnt[0], n = total < cap ? total : cap;
  // (a tuple the snapshot check could not decide is kept AND counted for a recheck)
  if (total + cnt[2] > nitems_all || cnt[1] > nitems_all)
    FAIL("kept %u, rechecked %u, removed %u of %u line pointers", total, cnt[1], cnt[2], nitems_all);
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t pg = items[i] >> 16, ln = items[i] & 0xffff;
    if (i && items[i] <= items[i - 1]) FAIL("items not ascending at %u", i);
    if (pg >= r.npages || (status[pg] & ~STROM_PAGE_RECHECK)) FAIL("item of page %u", pg);
    const uint8_t *page = pages + (size_t)pg * r.page_sz;
    const uint32_t lower = (uint32_t)page[12] | ((uint32_t)page[13] << 8);
    if (ln < 1 || ln > (lower - 24) / 4) FAIL("line number %u of %u", ln, (lower - 24) / 4);
  }
  if (count) {
    t->kept += total;
    t->rechecked += cnt[1];
    t->dropped += nitems_all - total;
  }
  if (items_out) items_out->assign(items.get(), items.get() + n);
  if (status_out) status_out->assign(status.get(), status.get() + r.npages);
  if (recheck_out) *recheck_out = cnt[1];
  return 0;
}

int project_all(const Record &r, const uint8_t *pages, const std::vector<uint32_t> &items,
                Totals *t) {
  const uint32_t n = (uint32_t)items.size();
  if (!n) return 0;
  std::unique_ptr<uint32_t[]> it(new uint32_t[n]);
  memcpy(it.get(), items.data(), 4 * (size_t)n);
  const uint32_t ncol = (uint32_t)r.desc.natts;
  std::unique_ptr<int32_t[]> att(new int32_t[ncol]);
  std::unique_ptr<uint64_t[]> values(new uint64_t[(size_t)ncol * n]);
  std::unique_ptr<uint8_t[]> valid(new uint8_t[(size_t)ncol * n]);
  uint32_t cols = 0;
  // every projectable column, descending: the entry sorts them
  for (int32_t k = (int32_t)ncol - 1; k >= 0; --k) {
    const int len = r.desc.attlen[k];
    if (len > 0 && len < 8 && len != 1 && len != 2 && len != 4) continue;
    att[cols++] = k;
  }
  if (!cols) return 0;
  memset(valid.get(), 0xEE, (size_t)ncol * n);
  const uint32_t cnt = n;
  const int rc = strom_heap_project_host(pages, r.page_sz, it.get(), &cnt, n, &r.desc, att.get(),
                                         cols, 0, values.get(), valid.get());
  if (rc) FAIL("project: rc %d", rc);
  for (uint32_t j = 0; j < cols; ++j)
    for (uint32_t i = 0; i < n; ++i) {
      const uint8_t ok = valid[(size_t)j * n + i];
      if (ok > 2) FAIL("valid %u", ok);
      if (ok && r.desc.attlen[att[j]] < 0) {
        const uint64_t v = values[(size_t)j * n + i], o = v >> 32, len = v & 0xffffffffu;
        const uint64_t pg = it[i] >> 16;
        if (o < pg * r.page_sz || o + len > (pg + 1) * r.page_sz)
          FAIL("varlena [%llu, +%llu) outside page %llu", (unsigned long long)o,
               (unsigned long long)len, (unsigned long long)pg);
      }
      ++t->projected;
    }
  return 0;
}

int run_pages(const Record &r, const uint8_t *src, std::mt19937_64 &rng, const Snapshot &sn,
              Totals *t, bool mutated) {
  // the pages in an allocation of exactly their size
  const size_t bytes = (size_t)r.npages * r.page_sz;
  std::unique_ptr<uint8_t[]> pages(new uint8_t[bytes]);
  memcpy(pages.get(), src, bytes);
  uint32_t max_items = 0;
  for (uint32_t pg = 0; pg < r.npages; ++pg) max_items += (r.page_sz - 24) / 4;
  bool first = true;
  for (int snap = 0; snap < 2; ++snap) {
    // hint-bit visibility at random; the checksum only where the page still is
    // as stamped (a mutant fails it before any tuple is looked at)
    const uint32_t flags = (uint32_t)(rng() & 2) | (mutated ? 0u : (uint32_t)(rng() & 1));
    const uint32_t cap = rng() % 4 == 0 ? (uint32_t)(rng() % 3) : max_items;
    std::vector<uint32_t> items, status;
    if (scan_once(r, pages.get(), 0, nullptr, snap, sn, cap, flags, &items, &status, nullptr, t,
                  first))
      return 1;
    if (first && mutated)
      for (uint32_t pg = 0; pg < r.npages; ++pg) {
        ++t->mutated;
        if (!(status[pg] & ~STROM_PAGE_RECHECK)) ++t->mutated_accepted;
      }
    first = false;
    for (const QualSet &qs : r.sets) {
      std::vector<uint32_t> i1, s1, i2, s2;
      uint32_t r1 = 0, r2 = 0;
      const bool fixed = qs.nfixed != 0xFFFFFFFFu, prog = qs.nprog != 0;
      if (fixed && scan_once(r, pages.get(), 1, &qs, snap, sn, max_items, flags, &i1, &s1, &r1, t,
                             true))
        return 1;
      if (prog && scan_once(r, pages.get(), 2, &qs, snap, sn, max_items, flags, &i2, &s2, &r2, t,
                            !fixed))
        return 1;
      if (fixed && prog && (i1 != i2 || s1 != s2 || r1 != r2))
        FAIL("the fixed list and the program disagree: %zu / %zu items, %u / %u rechecks",
             i1.size(), i2.size(), r1, r2);
      if (project_all(r, pages.get(), fixed ? i1 : i2, t)) return 1;
    }
  }
  return 0;
}

// a random mutation of the program's own: mostly behind the page header
void mutate(std::vector<uint8_t> &pg, uint32_t page_sz, uint32_t npages, std::mt19937_64 &rng) {
  const int n = 1 + (int)(rng() % 4);
  for (int k = 0; k < n; ++k) {
    uint8_t *page = pg.data() + (size_t)(rng() % npages) * page_sz;
    const uint32_t lower = (uint32_t)page[12] | ((uint32_t)page[13] << 8);
    const uint32_t nlp = lower >= 28 && lower <= page_sz ? (lower - 24) / 4 : 1;
    uint8_t *lp = page + 24 + 4 * (rng() % nlp);
    uint32_t w;
    memcpy(&w, lp, 4);
    const uint32_t off = w & 0x7fff;
    switch (rng() % 8) {
      case 0:                                      // a header byte
        page[8 + rng() % 12] ^= (uint8_t)(1u << (rng() % 8));
        break;
      case 1:                                      // a line pointer bit
        w ^= 1u << (rng() % 32);
        memcpy(lp, &w, 4);
        break;
      case 2:                                      // lp_len to the page's end, or past it
        w = (w & 0x1ffff) | (((page_sz - off + (uint32_t)(rng() % 3) - 1) & 0x7fff) << 17);
        memcpy(lp, &w, 4);
        break;
      case 3:                                      // t_hoff
        if (off + 24 <= page_sz) page[off + 22] = (uint8_t)(rng() % 5 ? 8 * (rng() % 8) : rng());
        break;
      case 4:                                      // natts, infomask
        if (off + 24 <= page_sz) page[off + 18 + rng() % 4] ^= (uint8_t)(1u << (rng() % 8));
        break;
      default: {                                   // a byte of the tuple's first 96
        const uint32_t at = off + 23 + (uint32_t)(rng() % 96);
        if (at < page_sz) page[at] = (uint8_t)(rng() % 3 ? rng() : (rng() % 2 ? 0x01 : 0x00));
      }
    }
  }
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: %s FILE ROUNDS [SEED]\n", argv[0]);
    return 2;
  }
  FILE *f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  std::vector<uint8_t> file;
  uint8_t chunk[65536];
  for (size_t n; (n = fread(chunk, 1, sizeof chunk, f)) > 0;) file.insert(file.end(), chunk, chunk + n);
  fclose(f);
  const int rounds = atoi(argv[2]);
  std::mt19937_64 rng(argc > 3 ? strtoull(argv[3], nullptr, 10) : 4321);
  Reader rd{file.data(), file.data() + file.size()};
  uint32_t magic = 0, nrec = 0;
  if (!rd.u32(&magic) || magic != 0x50414548u || !rd.u32(&nrec)) {
    fprintf(stderr, "not a heap fuzz input\n");
    return 2;
  }
  const Snapshot sn;
  Totals t;
  for (uint32_t i = 0; i < nrec; ++i) {
    Record r;
    uint32_t nsets = 0;
    if (!rd.u32(&r.page_sz) || !rd.u32(&r.npages) || !rd.u32(&r.mutant)) return 2;
    if (r.page_sz < 1024 || r.page_sz > 32768 || (r.page_sz & 1023) || !r.npages || r.npages > 64)
      return 2;
    r.pages.resize((size_t)r.npages * r.page_sz);
    if (!rd.take(r.pages.data(), r.pages.size()) || !rd.take(&r.desc, sizeof r.desc) ||
        !rd.u32(&nsets) || nsets > 256)
      return 2;
    r.sets.resize(nsets);
    for (QualSet &qs : r.sets) {
      if (!rd.u32(&qs.nfixed) || !rd.take(qs.fixed, sizeof qs.fixed) || !rd.u32(&qs.nprog)) return 2;
      if (qs.nprog > 4096) return 2;
      qs.prog.reset(new uint8_t[qs.nprog ? 32 * (size_t)qs.nprog : 1]);
      if (!rd.take(qs.prog.get(), 32 * (size_t)qs.nprog) || !rd.u32(&qs.pool_len)) return 2;
      if (qs.pool_len > (1u << 20)) return 2;
      qs.pool.reset(new uint8_t[qs.pool_len ? qs.pool_len : 1]);
      if (!rd.take(qs.pool.get(), qs.pool_len)) return 2;
      if (qs.nprog && strom_heap_prog_check(&r.desc, (const strom_heap_qual2 *)qs.prog.get(),
                                            qs.nprog, qs.pool.get(), qs.pool_len)) {
        fprintf(stderr, "record %u: a program fails its check\n", i);
        return 1;
      }
    }
    if (run_pages(r, r.pages.data(), rng, sn, &t, r.mutant != 0)) {
      fprintf(stderr, "record %u as read failed\n", i);
      return 1;
    }
    for (int k = 0; k < rounds; ++k) {
      std::vector<uint8_t> pg = r.pages;
      mutate(pg, r.page_sz, r.npages, rng);
      if (run_pages(r, pg.data(), rng, sn, &t, true)) {
        fprintf(stderr, "record %u, mutation round %d failed\n", i, k);
        return 1;
      }
    }
  }
  printf("heapscan_fuzz: %u records x %d rounds ok; pages accepted %ld rejected %ld, tuples kept %ld "
         "dropped %ld rechecked %ld, projected %ld; mutated pages %ld accepted %ld\n",
         nrec, rounds, t.accepted, t.rejected, t.kept, t.dropped, t.rechecked, t.projected,
         t.mutated, t.mutated_accepted);
  return 0;
}
