/*
 * strom/strom.h — C ABI of libstrom, the MI355X-native direct-storage
 * engine.  Everything a client needs: the ioctl-compatible entry points
 * (sessions stand in for open file descriptors on /proc/nvme-strom), engine
 * configuration, and the CDNA4 post-read kernels (verify, reorder, scan,
 * decompress, filter) that run on HBM-resident data.
 *
 * Return convention: 0 or a non-negative count on success, -errno on error
 * (never sets errno) — except nvme_strom_ioctl(), which mimics ioctl(2).
 */
#ifndef STROM_STROM_H
#define STROM_STROM_H

#include <stddef.h>
#include <stdint.h>

#include "strom/uapi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- sessions + dispatch ---------------------------------------------- */
const char *strom_version(void);
/* 0 = userspace engine, 1 = kernel module (/proc or /dev node present). */
int strom_provider(void);
int strom_open(void);                    /* new session id (> 0) */
int strom_close(int session);            /* reclaims failed tasks: count */
int strom_ioctl(int session, unsigned long cmd, void *arg);
/* v0.6-style wrapper (utils_common.h): lazily opened per-thread session,
 * returns 0 / -1 with errno set. */
int nvme_strom_ioctl(unsigned long cmd, const void *arg);

/* Synchronous "pread into HBM": [file_off, file_off+len) of fd lands at
 * offset of a mapped GPU range, through the same engine path as
 * MEMCPY_SSD2GPU + WAIT (page-cache pages included, in file order).
 * file_off and len must be 4 KiB multiples.  Returns len or -errno. */
long strom_pread_gpu(int session, unsigned long handle, size_t offset, int fd,
                     uint64_t file_off, uint64_t len);
/* QD1 latency probe: n strom_pread_gpu calls of len bytes at file_offs[i],
 * wall time of each in ns_out[i] (native loop, no caller overhead).
 * Returns 0 or the first failure's -errno. */
int strom_pread_gpu_lat(int session, unsigned long handle, size_t offset, int fd,
                        const uint64_t *file_offs, uint32_t n, uint64_t len, uint64_t *ns_out);
/* The same QD1 probe through the ioctl pair a v0.6 client issues
 * (MEMCPY_SSD2GPU of len/4096 chunks + MEMCPY_WAIT per read): task table,
 * residency probe and planner included.  len <= 1 MiB. */
int strom_ioctl_lat(int session, unsigned long handle, size_t offset, int fd,
                    const uint64_t *file_offs, uint32_t n, uint64_t len, uint64_t *ns_out);
/* The same probe split into phases: phase_ns[i*STROM_NPHASE + k] is the time
 * from the start of read i to the end of phase k, 0 when k was not reached:
 *   0 file lookup   1 chunk plan (residency probe + merge)   2 task + requests
 *   3 storage read   4 stores into HBM (BAR) or the SDMA copy   5 HDP flush
 *   6 request completion   7 WAIT returned (the total). */
#define STROM_NPHASE 8
int strom_pread_gpu_phases(int session, unsigned long handle, size_t offset, int fd,
                           const uint64_t *file_offs, uint32_t n, uint64_t len,
                           uint64_t *phase_ns);
/* The floor under those reads: O_DIRECT pread of len bytes at each offset
 * into aligned host memory (no engine, no HBM), ns per read. */
int strom_pread_raw_lat(int fd, const uint64_t *file_offs, uint32_t n, uint64_t len,
                        uint64_t *ns_out);
/* QD1 pairs, interleaved: a raw O_DIRECT pread (offs[2i]) and a
 * strom_pread_gpu (offs[2i+1]) per pair, order flipped every pair; ns each. */
int strom_pread_pair_lat(int session, unsigned long handle, size_t offset, int fd,
			 const uint64_t *file_offs, uint32_t npairs, uint64_t len,
			 uint64_t *ns_engine, uint64_t *ns_raw);

/* Host primitive costs (ns per call, mean of n) on this machine, for the
 * latency breakdown: {clock_gettime, rdtsc, fstat(fd), mincore 1 page of fd,
 * bare syscall, mutex lock+unlock, condvar notify} -> out[7]. */
int strom_host_costs(int fd, uint64_t *out, int n);
/* the engine's own steps of a synchronous read (registry lookup, freed-range
 * check, file cache, completion bookkeeping), ns per call; out[6..13] are a
 * 4 KiB BAR store and the first locked instruction after it,
 * for memcpy / whole-line non-temporal / the same last line first / rep movsb,
 * then the 4 KiB split over two cores (start to both halves drained) and
 * that split's hand-off alone -> out[16] */
int strom_engine_costs(unsigned long handle, int fd, uint64_t *out, int n);

/* Storage ceiling for a block size, no engine: `threads` io_uring rings,
 * each `qd` deep, O_DIRECT reads of `block` bytes at random aligned
 * offsets (or, `sequential`, each ring its own run in file order) into
 * host memory until `nreq` reads are done. */
int strom_raw_read_rate(int fd, uint64_t block, uint32_t nreq, uint32_t threads, uint32_t qd,
                        int sequential, double *iops, double *gibps);
/* The same rings reading exactly the requests (off[i], len[i]), 4 KiB
 * aligned, thread t taking the t-th contiguous share of the list: the
 * storage's rate for the access pattern an engine call produced. */
int strom_raw_read_list(int fd, const uint64_t *off, const uint32_t *len, uint32_t n,
                        uint32_t threads, uint32_t qd, int mode, double *iops, double *gibps);

/* dma-buf fd of the HIP allocation holding [va, va+len) and va's byte
 * offset inside it: what MAP_GPU_MEMORY registers with the kernel provider
 * (MAP_GPU_DMABUF).  The caller closes the fd. */
int strom_export_dmabuf(uint64_t va, uint64_t len, int *fd, uint64_t *offset);

/* Stripe set: a logical file of `size` bytes striped in `unit`-byte
 * stripes (multiple of 4 KiB) over n member files (stripe s in member
 * s % n at offset (s / n) * unit) — one member per SSD aggregates them
 * without md.  Returns a pseudo descriptor usable as file_desc for
 * CHECK_FILE / SSD2GPU / SSD2RAM / strom_pread_gpu until closed; -ERANGE
 * when a member is too short.  Userspace provider only. */
int strom_stripe_open(const int *fds, uint32_t n, uint32_t unit, uint64_t size);
int strom_stripe_close(int sfd);
/* Registered file (as io_uring's registered files): the descriptor is
 * resolved once; the returned id is accepted wherever a file descriptor is
 * and skips the per-read identity check (fstat / kcmp).  The engine reads
 * through descriptors of its own: the caller may close fd.  An id lives
 * until strom_unregister_file() or an engine reset (-EBADF after). */
int strom_register_file(int fd);
int strom_unregister_file(int rfd);

/* SSD2RAM destinations: mmap (MAP_SHARED, read/write) `length` bytes of an
 * ALLOC_DMA_BUFFER fd through the engine, so the range is found in the
 * registry's address index; NULL + errno on failure.  Unmap with
 * strom_dmabuf_munmap.  A caller's own mmap of the fd works too (looked up
 * by one PROCMAP_QUERY per request). */
void *strom_dmabuf_mmap(int fd, size_t length);
int strom_dmabuf_munmap(void *addr, size_t length);
/* Drop DMA buffers no fd and no mapping of the process refers to any more;
 * returns how many stay registered. */
int strom_dmabuf_gc(void);
/* Mappings detached because their allocation was freed or replaced. */
long strom_gpu_detached(void);
/* Bytes of a mapping the CPU can store into through the large BAR (0: none;
 * small reads then go staging -> SDMA / ingest grid instead). */
long strom_gpu_bar_bytes(unsigned long handle);

/* Placement facts of a file for GPU<->SSD affinity (CHECK_FILE tells
 * only the NUMA node): the backing disk, its members (md raid0) and the
 * PCI function of each member's controller (NVMe, or whatever PCI device
 * the disk hangs off; "" when unknown).  nmembers = 0 for a virtual filesystem (overlay, tmpfs). */
#define STROM_TOPO_MAX_MEMBERS 16
typedef struct strom_file_topo {
  uint32_t dev_major, dev_minor; /* st_dev of the file */
  int32_t numa_node;
  uint32_t nmembers;
  char fs_name[16];
  char disk[32];
  char member_disk[STROM_TOPO_MAX_MEMBERS][32];
  char member_pci[STROM_TOPO_MAX_MEMBERS][16];
} strom_file_topo;
int strom_file_topology(int fd, strom_file_topo *out);
/* PCI function "dddd:bb:dd.f" of a HIP device (no GPU init past the
 * runtime's own); -ENODEV without one. */
int strom_gpu_pci_bdf(int device, char *buf, size_t len);

/* HBM ingest grid of a device (the persistent GPU pull kernel that moves
 * staged reads into HBM): out[4] = {available, grid launches, descriptors
 * posted, descriptors outstanding}.  -ENODEV when it cannot run there. */
int strom_ingest_info(int device, uint64_t *out);

/* Worker phase attribution (config io_prof=1): out[0] workers, out[1] TSC
 * kHz, out[2..12] TSC cycles summed over the workers per phase (idle, take,
 * start, submit, reap, bar, post, hdp, finish, retire, wait), out[13..17]
 * counts (requests, batches, io_uring_enter calls, sleeps, HBM
 * descriptors), out[18..21] the submitting side (SSD2GPU/SSD2RAM calls and
 * TSC cycles planning, building requests, handing them over).  reset != 0
 * zeroes them.  Returns the number of u64 written (22) or -errno. */
int strom_io_prof(uint64_t *out, int nout, int reset);

/* ---- configuration (env STROM_<KEY> is read at first use) ------------- */
int strom_config_set(const char *key, const char *value);
int strom_config_get(const char *key, char *buf, size_t buflen);
/* Tear the engine down (waits for in-flight I/O); next call re-creates it
 * with the current configuration. */
int strom_engine_reset(void);

/* ---- fault injection (fake + real backends; CPU tests) ---------------- */
/* Fail the n-th storage request after this call (1-based) with -err; 0
 * disables.  short_at makes the n-th request read `short_bytes` less. */
int strom_fault_inject(long fail_at, int err, long short_at, int short_bytes,
                       int delay_us);

/* Fake namespace backend (backend=fake): completions come back in a seeded
 * random order.  Sets the seed (0 keeps it; takes effect at the next
 * engine reset) and reads the completion / out-of-order counters. */
int strom_fake_backend(uint64_t seed, uint64_t *completions, uint64_t *reordered);

/* ---- host helpers ------------------------------------------------------ */
/* Bytes of a file range resident in the page cache (mincore). */
long strom_resident_bytes(int fd, uint64_t offset, uint64_t length);
/* Drop clean page-cache pages of a file (posix_fadvise DONTNEED). */
int strom_evict_file(int fd);
/* CRC32C (Castagnoli) on the host, same convention as the GPU kernels. */
uint32_t strom_crc32c_host(uint32_t crc, const void *buf, size_t len);
/* md raid0 remap for a described geometry (tests + kmod parity). */
int strom_raid0_map(const uint64_t *zone_end, const uint64_t *zone_dev_start,
                    const int *zone_nb_dev, int nzones,
                    uint32_t chunk_sects, const uint64_t *data_offset,
                    int raid_disks, uint64_t sector, uint32_t nr_sects,
                    int *member, uint64_t *member_sector);
/* Host LZ4 / snappy block codecs (test-data generation + CPU reference). */
long strom_lz4_compress_host(const void *src, size_t n, void *dst, size_t cap);
long strom_lz4_decompress_host(const void *src, size_t n, void *dst, size_t cap);
long strom_snappy_compress_host(const void *src, size_t n, void *dst, size_t cap);
long strom_snappy_decompress_host(const void *src, size_t n, void *dst, size_t cap);

/* ---- CDNA4 kernels (device pointers, hipStream_t passed as void*) ----- */
int strom_gpu_count(void);
/* Per-chunk CRC32C: out[i] = crc32c(in + i*chunk, min(chunk, n - i*chunk)). */
int strom_crc32c_chunks(const void *d_in, uint64_t nbytes, uint32_t chunk,
                        uint32_t *d_out, void *stream);
/* Fold per-chunk CRCs (equal chunk sizes, last may be short) into the CRC
 * of the whole buffer; d_out is one u32. */
int strom_crc32c_combine(const uint32_t *d_crcs, uint32_t nchunks,
                         uint32_t chunk, uint64_t nbytes, uint32_t *d_out,
                         void *stream);
/* Chunk scatter: dst + pos[i]*chunk <- src + i*chunk, i < n. */
int strom_chunk_scatter(const void *d_src, void *d_dst, const uint32_t *d_pos,
                        uint32_t n, uint32_t chunk, void *stream);
/* Chunk gather: dst + i*chunk <- src + idx[i]*chunk. */
int strom_chunk_gather(const void *d_src, void *d_dst, const uint32_t *d_idx,
                       uint32_t n, uint32_t chunk, void *stream);
/* Compare against a 32-bit pattern / a reference buffer: out[0] = mismatching
 * 4-byte words, out[1] = first mismatching byte offset (or ~0). */
int strom_verify_pattern(const void *d_buf, uint64_t nbytes, uint32_t pattern,
                         uint64_t *d_out, void *stream);
int strom_verify_equal(const void *d_a, const void *d_b, uint64_t nbytes,
                       uint64_t *d_out, void *stream);
int strom_fill_pattern(void *d_buf, uint64_t nbytes, uint32_t pattern,
                       void *stream);

/* The full HeapTupleSatisfiesMVCC inputs (heapam_visibility.c): snapshot
 * (xmin, xmax, xip, subxip / suboverflowed), the scanning transaction's own
 * xids and command id, and windows of the SLRU logs — pg_xact (2 bits per
 * xid from clog_base), pg_subtrans (parent xid per xid from subtrans_base),
 * pg_multixact offsets (member offset per multixact from mx_base, n + 1
 * entries: the last is the next offset) and members (PostgreSQL's page
 * layout: 409 groups of 4 flag bytes + 4 xids per 8 KiB page, from member
 * offset mxm_base).  Transaction ids compare modulo 2^32. */
struct strom_pg_mvcc {
	uint32_t xmin, xmax;
	const uint32_t *xip;
	uint32_t nxip;
	uint32_t suboverflowed;
	const uint32_t *subxip;
	uint32_t nsubxip;
	uint32_t curcid;
	const uint32_t *curxids;  /* the scanning transaction: top xid + its subxacts */
	uint32_t ncurxids;
	uint32_t clog_base;
	const uint8_t *clog;
	uint64_t clog_n;
	const uint32_t *subtrans;
	uint32_t subtrans_base, subtrans_n;
	const uint32_t *mx_offsets;
	uint32_t mx_base, mx_n;
	const uint8_t *mx_members;
	uint64_t mxm_n;
	uint32_t mxm_base, pad;
};

/* PostgreSQL heap pages (8 KiB by default). */
struct strom_heap_scan_args {
	const void *pages;       /* device: npages * page_sz bytes */
	uint32_t npages;
	uint32_t page_sz;
	uint32_t flags;          /* STROM_HEAP_* */
	int32_t  attr_off;       /* byte offset of the filtered int column in
	                            tuple data (after t_hoff), -1 = no filter */
	int32_t  attr_width;     /* 4 or 8 */
	int64_t  lo, hi;         /* keep rows with lo <= v <= hi */
	uint32_t *out_items;     /* device: (page << 16) | lineno, capacity below */
	uint32_t out_cap;
	uint32_t *out_count;     /* device: u32[1], total qualifying */
	uint32_t *page_status;   /* device: per page bitfield (STROM_PAGE_*) */
	uint32_t blkno_base;     /* block number of page 0 (checksum input) */
	const uint32_t *blknos;  /* device, optional: block number per page
	                            (pages landed out of order); overrides
	                            blkno_base + page */
};
#define STROM_HEAP_VERIFY_CHECKSUM 1u
#define STROM_HEAP_SKIP_INVISIBLE  2u   /* honour xmin/xmax hint bits */
#define STROM_PAGE_BAD_HEADER  1u
#define STROM_PAGE_BAD_CHECKSUM 2u
#define STROM_PAGE_EMPTY       4u
int strom_heap_scan(const struct strom_heap_scan_args *a, void *stream);

/* General tuple deforming + qualifier lists (the reference hands every tuple
 * to ExecScan, which deforms it and evaluates any qual list:
 * pgsql/nvme_strom.c:1137-1143, :1054-1092).  A tuple descriptor in
 * PostgreSQL's pg_attribute terms locates every attribute: the null bitmap
 * (HEAP_HASNULL, t_bits), attalign padding, fixed lengths, and varlena
 * headers (1-byte short, 4-byte, 1-byte-external TOAST pointers).  Tuples
 * with fewer stored attributes than the descriptor (ALTER TABLE ADD COLUMN)
 * read the missing ones as NULL. */
#define STROM_HEAP_MAX_ATTS  64
#define STROM_HEAP_MAX_QUALS 8
struct strom_heap_tupdesc {
	int32_t natts;
	int16_t attlen[STROM_HEAP_MAX_ATTS];    /* > 0 fixed, -1 varlena, -2 cstring */
	uint8_t attalign[STROM_HEAP_MAX_ATTS];  /* 1, 2, 4 or 8 ('c' 's' 'i' 'd') */
	int16_t cacheoff[STROM_HEAP_MAX_ATTS];  /* offset after t_hoff when every earlier
	                                           attribute is fixed-length (tuples without
	                                           nulls), else -1 (attcacheoff) */
};
#define STROM_QUAL_INT_RANGE    1  /* lo <= v <= hi, v an int of attlen 1/2/4/8 */
#define STROM_QUAL_FLOAT_RANGE  2  /* lo <= v <= hi as doubles (bit patterns in lo/hi),
                                      v a float4 / float8 */
#define STROM_QUAL_IS_NULL      3
#define STROM_QUAL_NOT_NULL     4
#define STROM_QUAL_TEXT_EQ      5  /* varlena bytes == cbytes[0..nconst) */
#define STROM_QUAL_TEXT_PREFIX  6  /* varlena bytes start with cbytes[0..nconst) */
#define STROM_QUAL_INT_IN       7  /* v in { ((int64_t *)cbytes)[0..nconst) } (<= 4) */
struct strom_heap_qual {
	int16_t attno;       /* 0-based column */
	uint8_t kind;        /* STROM_QUAL_* */
	uint8_t nconst;      /* TEXT_*: constant length (<= 32); INT_IN: values (<= 4) */
	uint32_t pad;
	int64_t lo, hi;
	uint8_t cbytes[32];
};
/* A text qualifier meets a compressed or out-of-line (TOAST) value: the GPU
 * cannot decide it, the tuple is not emitted and its page is flagged
 * STROM_PAGE_RECHECK for the host to re-evaluate. */
#define STROM_PAGE_RECHECK     8u
#define STROM_QUAL_TEXT_IN      8  /* varlena bytes == one of nconst constants */
#define STROM_QUAL_NUMERIC_RANGE 9 /* lo <= v <= hi, v a PostgreSQL numeric */
#define STROM_QUAL2_FALSE 0x80   /* strom_heap_qual2.flags: the qual is constant false */
/* A qualifier of a program (strom_heap_scan2_args.prog): quals with the
 * same clause id are ORed and contiguous, clauses are ANDed (CNF); any
 * number of either.  Constants live in a device pool:
 *   TEXT_EQ / TEXT_PREFIX  nconst bytes at coff (any length)
 *   INT_IN                 nconst int64 at coff (any count)
 *   TEXT_IN                nconst (uint32 offset, uint32 length) at coff
 *   NUMERIC_RANGE          constants at pool offsets lo and hi: uint16 kind
 *                          (0 finite, 1 NaN, 2 +inf, 3 -inf), uint16 sign
 *                          (0 / 1 negative), int16 weight, uint16 ndigits,
 *                          int16 base-10000 digits (no leading / trailing 0s)
 * flags (NUMERIC_RANGE): 1 no lower bound, 2 no upper bound, 4 lower
 * strict, 8 upper strict. */
struct strom_heap_qual2 {
	int16_t attno;
	uint8_t kind;
	uint8_t flags;
	uint32_t clause;
	uint32_t nconst;
	uint32_t coff;
	int64_t lo, hi;
};
struct strom_heap_scan2_args {
	struct strom_heap_scan_args base;     /* base.attr_off must be -1 */
	struct strom_heap_tupdesc desc;
	int32_t nquals;                       /* ANDed; NULL never qualifies
	                                         except for IS_NULL */
	struct strom_heap_qual quals[STROM_HEAP_MAX_QUALS];
	uint32_t *recheck_count;              /* device, optional: undecidable tuples */
	/* program mode (prog != NULL; quals / nquals unused): nprog quals in
	 * device memory, their constants in cpool (cpool_len bytes) */
	const struct strom_heap_qual2 *prog;
	const uint8_t *cpool;                 /* 8-aligned constants, cpool_len % 8 == 0 */
	uint32_t nprog, cpool_len;
	/* Snapshot visibility on the device (mvcc_on != 0): every LP_NORMAL
	 * tuple of a page that is not PD_ALL_VISIBLE — and, with mvcc_pages,
	 * whose byte is nonzero (the visibility map said "not all-visible") — is
	 * checked with HeapTupleSatisfiesMVCC's rules (strom_pg_tuple_visible's,
	 * pgsql/nvme_strom.c:907-936 runs them per buffer-manager tuple).  An
	 * invisible tuple is dropped and counted in mvcc_removed[0]; one the
	 * inputs cannot decide (combo cid, an xid / multixact outside the
	 * windows) is kept, as the host check keeps it, and its page flagged
	 * STROM_PAGE_RECHECK.  mvcc's pointers are DEVICE memory, and xip /
	 * subxip / curxids must be sorted ascending (binary-searched). */
	struct strom_pg_mvcc mvcc;
	const uint8_t *mvcc_pages;            /* device, optional: per page */
	uint32_t *mvcc_removed;               /* device, optional: u32[1] */
	uint32_t mvcc_on;
	/* optional: bit k set when xid mvcc.xmin + k is running for the
	 * snapshot (in xip, or in subxip unless suboverflowed), k < running_bits
	 * = xmax - xmin: XidInMVCCSnapshot's list searches become one load */
	uint32_t mvcc_running_bits;
	const uint32_t *mvcc_running;
};
int strom_heap_scan2(const struct strom_heap_scan2_args *a, void *stream);
/* strom_heap_scan (the fixed-offset int predicate) with the device snapshot
 * check above; m holds device pointers (NULL m: hint bits only). */
int strom_heap_scan_mvcc(const struct strom_heap_scan_args *a, const struct strom_pg_mvcc *m,
                         const uint8_t *mvcc_pages, uint32_t *mvcc_removed,
                         uint32_t *recheck_count, const uint32_t *running,
                         uint32_t running_bits, void *stream);
/* The host ("buffer manager") path for blocks checked on the CPU: each
 * block blocks[i] is read (pread of page_sz bytes at (block % relseg_blocks)
 * * page_sz; relseg_blocks 0: no modulo) into stage + i * page_sz, a short
 * read zero-filled; with verify_checksum its checksum is tested first and,
 * when valid, re-stamped after the edit (as ReadBuffer + a hint-bit write);
 * then the tuples m hides are marked LP_UNUSED.  recheck_flags[i] (optional)
 * = 1 when the block holds tuples the inputs cannot decide.  Returns the
 * tuples removed, or -errno of a failed read. */
long strom_pg_read_check_pages(int fd, const uint32_t *blocks, uint32_t n, uint32_t relseg_blocks,
                               uint32_t page_sz, void *stage, const struct strom_pg_mvcc *m,
                               int verify_checksum, uint8_t *recheck_flags);
/* Checks a program and its pool (host copies of what prog / cpool hold)
 * before a launch: kinds against the attributes, contiguous clauses, every
 * constant (IN tables and the text entries they name, numeric digits)
 * inside the pool.  0 or -EINVAL. */
int strom_heap_prog_check(const struct strom_heap_tupdesc *d, const struct strom_heap_qual2 *prog,
			  uint32_t n, const uint8_t *pool, uint32_t pool_len);
/* Projection of one attribute of the tuples `items` (page << 16 | lineno,
 * as strom_heap_scan writes them) names: values[i] (8 bytes: the int
 * sign-extended, float4 widened to double, varlena: (offset in pages <<
 * 32 | data length) of the uncompressed inline bytes) and valid[i] (0 NULL,
 * 1 value, 2 compressed / out-of-line varlena).  *d_count (device) is the
 * number of items; at most cap are read. */
int strom_heap_project(const void *pages, uint32_t page_sz, const uint32_t *items,
                       const uint32_t *d_count, uint32_t cap,
                       const struct strom_heap_tupdesc *desc, int attno, int as_float,
                       uint64_t *values, uint8_t *valid, void *stream);
/* several attributes in one deform walk per tuple: values / valid are
 * [ncol][cap], column j as float64 when bit j of float_mask is set */
int strom_heap_project_n(const void *pages, uint32_t page_sz, const uint32_t *items,
                         const uint32_t *d_count, uint32_t cap,
                         const struct strom_heap_tupdesc *desc, const int32_t *attnos,
                         uint32_t ncol, uint64_t float_mask, uint64_t *values, uint8_t *valid,
                         void *stream);
/* What the heap scan and the projection take for a tuple, in one place (the
 * kernels, their host copy and the Python models in utils/pgpage.py and
 * utils/pgtuple.py follow it; docs/ARCHITECTURE.md, "Malformed heap input"):
 * a line pointer is followed when it is LP_NORMAL, lp_len >= 23, lp_off >= 24,
 * lp_off + lp_len <= page_sz and lp_off is MAXALIGNed (lp_off & 7 == 0, as
 * PageAddItem writes it; the aligned readers rely on it).  Every read of a
 * tuple is bounds-checked against lp_len first and wide reads touch only the
 * aligned 4-byte words that hold a byte of the datum, so nothing past
 * `pages + npages * page_sz` is read: `pages` needs no slack, only 4-byte
 * alignment of its start.
 *
 * The host copy of the scan kernels: the same per-tuple code (page header
 * checks, checksum, deformer, qualifier evaluators, snapshot check) run over
 * the pages in order, one tuple at a time.  Every pointer of *g — pages,
 * outputs, prog / cpool, the mvcc lists — is HOST memory; out_items comes out
 * ascending.  gen selects the evaluator: 0 the fixed-offset int predicate of
 * strom_heap_scan (base.attr_off / lo / hi; desc and quals unused), 1 the
 * fixed AND list (prog must be NULL), 2 the program (prog != NULL, checked
 * here with strom_heap_prog_check).  Argument checks are those of the device
 * entries; recheck_count / mvcc_removed are added to, as on the device. */
int strom_heap_scan2_host(const struct strom_heap_scan2_args *g, int gen);
/* strom_heap_project_n on host memory (*count items, at most cap read) */
int strom_heap_project_host(const void *pages, uint32_t page_sz, const uint32_t *items,
                            const uint32_t *count, uint32_t cap,
                            const struct strom_heap_tupdesc *desc, const int32_t *attnos,
                            uint32_t ncol, uint64_t float_mask, uint64_t *values, uint8_t *valid);
/* The scan's launch shape for npages pages of page_sz bytes: workgroups, and
 * pages per wave per output reservation (a workgroup of 4 waves takes
 * 4 * pages_per_wave pages per trip of its grid-stride loop).  The launch
 * itself calls this.  0 or -EINVAL. */
int strom_heap_scan_geometry(uint32_t page_sz, uint32_t npages, uint32_t *grid,
                             uint32_t *pages_per_wave);
uint16_t strom_pg_checksum_host(const void *page, uint32_t blkno,
                                uint32_t page_sz);
/* Per-tuple MVCC check of a heap page against a snapshot (xmin, xmax,
 * in-progress xids) and a commit log (pg_xact layout, 2 bits per xid):
 * invisible LP_NORMAL tuples are marked LP_UNUSED in place, as the
 * reference does before copying buffer-manager blocks into its chunk
 * (pgsql/nvme_strom.c:896-940).  PD_ALL_VISIBLE pages are left alone.
 * Returns the tuples removed. */
long strom_pg_apply_snapshot(void *page, uint32_t page_sz, uint32_t snap_xmin, uint32_t snap_xmax,
                             const uint32_t *xip, uint32_t nxip, const uint8_t *clog,
                             uint64_t clog_xids);
/* The same in-place marking with the full rules; tuples the inputs cannot
 * decide (a combo command id of the scanning transaction, an xid / multixact
 * outside the log windows) are kept and their line numbers (1-based)
 * written to recheck[] (up to cap), *nrecheck = their count.  Returns the
 * tuples removed, or -22 for a page that is not a heap page. */
long strom_pg_apply_mvcc(void *page, uint32_t page_sz, const struct strom_pg_mvcc *m,
                         uint16_t *recheck, uint32_t cap, uint32_t *nrecheck);
/* one tuple header: 1 visible, 0 not, -1 undecided */
int strom_pg_tuple_visible(const void *tuple_header, const struct strom_pg_mvcc *m);
/* fetch-and-add on shared memory (cross-process scan cursors) */
uint64_t strom_atomic_fetch_add_u64(uint64_t *addr, uint64_t v);
int strom_atomic_cas_u64(uint64_t *addr, uint64_t expect, uint64_t desired);
uint64_t strom_atomic_load_u64(const uint64_t *addr);

/* LZ4 / snappy raw-block batch decode: one block per wavefront. */
struct strom_decomp_desc {
	uint64_t src_off;      /* into d_src */
	uint64_t dst_off;      /* into d_dst */
	uint32_t src_len;
	uint32_t dst_len;      /* exact decoded size (or capacity) */
};
#define STROM_CODEC_LZ4    1
#define STROM_CODEC_SNAPPY 2
#define STROM_CODEC_COPY   3   /* stored block */
#define STROM_CODEC_LZ4_FRAME     4  /* LZ4 frame data blocks (after header) */
#define STROM_CODEC_LZ4_FRAME_BCS 5  /*   ... with 4-byte block checksums */
#define STROM_CODEC_ARROW_LZ4     6  /* Arrow IPC buffer: i64 length (-1 = raw) + LZ4 frame */
#define STROM_CODEC_ZSTD          7  /* Zstandard frame(s) (RFC 8878) */
#define STROM_CODEC_ARROW_ZSTD    8  /* Arrow IPC buffer: i64 length (-1 = raw) + zstd frame */
/* status[i] = decoded bytes, or -1 malformed / -2 overflow / -3 distance */
int strom_decompress(int codec, const void *d_src, void *d_dst,
                     const struct strom_decomp_desc *d_desc, uint32_t nblocks,
                     int32_t *d_status, void *stream);

/* Zstandard streams, one wavefront each (csrc/kernels/zstd.hip).  scratch:
 * 128 KiB of decoded literals per resident workgroup (NULL: a per-stream
 * buffer kept by the library).  strom_decompress() routes codecs 7/8 here. */
int strom_decompress_zstd(int codec, const void *d_src, void *d_dst,
                          const struct strom_decomp_desc *d_desc, uint32_t nstreams,
                          int32_t *d_status, void *scratch, uint64_t scratch_bytes,
                          void *stream);
/* the same with the decoder chosen by the caller: mode -1 the library's
 * choice, 0 one wave per stream, 1 frame-parallel (a frame's blocks on the
 * waves of a workgroup) */
int strom_decompress_zstd_mode(int codec, const void *d_src, void *d_dst,
                               const struct strom_decomp_desc *d_desc, uint32_t nstreams,
                               int32_t *d_status, void *scratch, uint64_t scratch_bytes,
                               void *stream, int mode);
/* decoder choice for strom_decompress_zstd: -1 by stream count (default),
 * 0 / 1 forced; returns the previous setting */
int strom_zstd_fp_mode(int mode);
/* buffers kept per (device, stream) by the zstd decoders (literal slots,
 * lane-parallel entry pools) */
uint32_t strom_zstd_scratch_keep(void);
/* free the library-kept zstd scratch (after the streams' last decodes) */
int strom_zstd_release(void);
/* the same decode on the CPU (the kernel's phases lane by lane) */
int strom_zstd_host(int codec, const uint8_t *src, uint32_t src_len, uint8_t *dst, uint32_t cap);

/* Columnar filter: bitmap[i/64] bit i%64 = valid(i) && lo <= v[i] <= hi,
 * the comparison exact against the double bounds (strom_filter_bounds). */
#define STROM_COL_I32 1
#define STROM_COL_I64 2
#define STROM_COL_F32 3
#define STROM_COL_F64 4
/* The bounds the range filters compare with, in the column's own type
 * (host; *lo_out / *hi_out receive one value of that type): integers
 * ceil(lo) and floor(hi) clamped to the type, F32 the smallest float >= lo
 * and the largest <= hi.  Returns 1, or 0 when no value can qualify (NaN on
 * either side, lo > hi, the range past one end of the type): the bounds are
 * then (1, 0) and the filters write zero words, count unchanged.  -22: type. */
int strom_filter_bounds(int type, double lo, double hi, void *lo_out, void *hi_out);
int strom_column_filter(int type, const void *d_values, const uint8_t *d_valid,
                        uint64_t n, double lo, double hi, uint64_t *d_bitmap,
                        uint64_t *d_count, void *stream);
/* Compact selected row indices from a bitmap (stable order). */
int strom_bitmap_to_indices(const uint64_t *d_bitmap, uint64_t n,
                            uint32_t *d_out, uint64_t *d_count, void *stream);

/* Batched scan over many record batches in ONE launch each, counts kept on
 * the device (no host sync per batch).  Batch b's rows occupy bitmap words
 * [word_base, word_base + ceil(nrows/64)) (every batch starts on a fresh
 * word); values / valid are device addresses (valid = 0: no nulls; Arrow
 * LSB-first bits, readable as whole 64-bit words). */
struct strom_filter_batch {
	uint64_t values;
	uint64_t valid;
	uint64_t nrows;
	uint64_t word_base;
	uint64_t row_base;     /* global row id of the batch's first row */
};
/* *d_count += selected rows (the caller zeroes it once per scan). */
int strom_column_filter_batched(int type, const struct strom_filter_batch *d_batches,
                                uint32_t nbatches, uint64_t nwords, double lo, double hi,
                                uint64_t *d_bitmap, uint64_t *d_count, void *stream);
/* Append the global row ids (int64, batch row_base + local row) of the set
 * bits to d_out at the device-side cursor *d_total, which advances by the
 * number appended: scans of successive groups fill one output in order. */
int strom_bitmap_to_rows(const uint64_t *d_bitmap, uint64_t nwords,
                         const struct strom_filter_batch *d_batches, uint32_t nbatches,
                         int64_t *d_out, uint64_t *d_total, void *stream);
/* Qualifier lists: combine != 0 ANDs the predicate into the existing
 * bitmap words (count = rows left selected). */
int strom_column_filter_batched2(int type, const struct strom_filter_batch *d_batches,
                                 uint32_t nbatches, uint64_t nwords, double lo, double hi,
                                 uint64_t *d_bitmap, uint64_t *d_count, int combine, void *stream);
/* bitmap_to_rows + projection: d_proj (same batches, another column's
 * values/valid pointers) non-NULL gathers each selected row's value (width 1,
 * 2, 4, 8 or 16 bytes) into d_pout[pos] and, when d_pvalid, its validity (0/1). */
int strom_bitmap_to_rows_proj(const uint64_t *d_bitmap, uint64_t nwords,
                              const struct strom_filter_batch *d_batches, uint32_t nbatches,
                              int64_t *d_out, uint64_t *d_total,
                              const struct strom_filter_batch *d_proj, uint32_t width,
                              void *d_pout, uint8_t *d_pvalid, void *stream);

/* General column qualifiers (Arrow scans; nvme_strom_amd/ops/colpred.py
 * compiles the predicates).  Storage types beyond STROM_COL_I32..F64: */
#define STROM_COL_I8 5
#define STROM_COL_I16 6
#define STROM_COL_U8 7
#define STROM_COL_U16 8
#define STROM_COL_U32 9
#define STROM_COL_U64 10
#define STROM_COL_BOOL 11   /* bit-packed values */
#define STROM_COL_STR32 12  /* utf8/binary: int32 offsets in values, bytes in aux */
#define STROM_COL_STR64 13  /* large utf8/binary: int64 offsets */
#define STROM_COL_DEC128 14 /* decimal128: 16-byte two's complement (value x 10^scale);
                               RANGES bounds are 16-byte pairs */
/* operators */
#define STROM_QOP_RANGES 1     /* v in one of nconst inclusive ranges: sorted, disjoint
                                  (lo, hi) pairs of int64 (U64: uint64; floats: double) */
#define STROM_QOP_STR_IN 2     /* the string equals one of nconst constants */
#define STROM_QOP_STR_PREFIX 3 /* starts with one of nconst constants */
#define STROM_QOP_LUT 4        /* index v < nconst with bit v of the uint32 LUT words set
                                  (dictionary-encoded columns) */
#define STROM_QOP_VALID 5      /* the row is not null (NEGATE: is null) */
#define STROM_QOP_STR_RANGES 6 /* bytewise-lexicographic ranges: per range two bounds of
                                  (start, len, mode) in offs, mode 0 unbounded,
                                  1 inclusive, 2 exclusive */
#define STROM_QOP_STR_LIKE 7   /* SQL LIKE: the string matches one of nconst patterns
                                  (csrc/kernels/collike.hip).  A pattern is its segments,
                                  the pieces between '%'; a segment is literal pieces with
                                  runs of '_' before and after them.  consts: the literal
                                  bytes, every piece starting 4-aligned.  offs, uint32 words:
                                    offs[k], k < nconst: word index of pattern k's record
                                    pattern: flags (STROM_LIKE_HEAD | STROM_LIKE_TAIL),
                                             least bytes of a match, nseg,
                                             then nseg word indexes of segment records
                                    segment: least bytes, npiece, '_' after the last piece,
                                             then npiece x ('_' before it, start in
                                             consts, length > 0)
                                  With HEAD the first segment starts at the row's first
                                  byte, with TAIL the last one ends at its last; no segment
                                  and both flags: only the empty string; no segment and no
                                  flag: every row. */
#define STROM_LIKE_HEAD 1
#define STROM_LIKE_TAIL 2
#define STROM_QUAL_NEGATE 1    /* NOT of the comparison (still false for nulls) */
#define STROM_QUAL_NAN 2       /* floats: NaN also matches (IN-lists holding NaN) */
#define STROM_QUAL_LIKE_WILD 4 /* STR_LIKE: some segment holds a '_' (without it the
                                  kernel runs its pure byte-search instantiation) */
#define STROM_QUAL_LIKE_UTF8 8 /* STR_LIKE: '_' is one code point, a byte and every
                                  0x80-0xBF byte directly after it (else one byte) */
/* STR_LIKE: a row with more than this many bytes to search for a pattern's
 * middle segments (a long row, less what the anchored head and tail took) is
 * matched one row per wave, the 64 lanes testing 64 candidate positions of a
 * searched segment, instead of one row per lane (STROM_LIKE_LONG_ROW in the
 * environment overrides it: the knob of tools/kbench.py) */
#define STROM_LIKE_LONG_ROW 256
struct strom_col_qual {
	int32_t type;
	int32_t op;
	uint32_t flags;
	uint32_t nconst;
	uint64_t consts;       /* device: ranges / string blob / LUT words */
	uint64_t offs;         /* device: strings, (start, len) uint32 pairs; starts 4-aligned */
	uint64_t const_bytes;  /* bytes at consts (staged in LDS, <= 64 KiB) */
	uint64_t offs_bytes;
};
/* strom_filter_batch + aux (the character data of a string column, aux_len
 * bytes: a row whose offsets are negative, decreasing or end past it is
 * selected by no string operator, NEGATE or not, and is never followed; it
 * still counts for STROM_QOP_VALID) */
struct strom_qual_batch {
	uint64_t values;
	uint64_t valid;
	uint64_t nrows;
	uint64_t word_base;
	uint64_t row_base;
	uint64_t aux;
	uint64_t aux_len;
};
/* bitmap[w] = (pred_bits | (d_or ? d_or[w] : 0)) & (and_dst ? bitmap[w] : ~0);
 * *d_count += popcount of the words written.  A CNF qualifier list is a
 * sequence of these launches (OR within a clause, AND across clauses). */
int strom_column_qual(const struct strom_col_qual *q, const struct strom_qual_batch *d_batches,
                      uint32_t nbatches, uint64_t nwords, uint64_t *d_bitmap,
                      const uint64_t *d_or, int and_dst, uint64_t *d_count, void *stream);
/* STROM_QOP_STR_LIKE of strom_column_qual on the CPU: the same row matcher
 * over host pointers (q->consts, q->offs and the batches' buffers in host
 * memory; the operands are checked, -22 for a record outside offs or a piece
 * outside consts).  As on the device the character buffer is read in aligned
 * dwords, so it is 4-byte aligned and readable up to the dword that holds
 * its last byte. */
int strom_column_like_host(const struct strom_col_qual *q, const struct strom_qual_batch *batches,
                           uint32_t nbatches, uint64_t nwords, uint64_t *bitmap,
                           const uint64_t *or_src, int and_dst, uint64_t *count);
/* bitmap_to_rows with a utf8/binary column projected (d_strtab: its
 * strom_qual_batch rows, offsets of owidth 4 or 8 bytes): each selected row's
 * characters are appended at the device cursor *d_char_cursor in d_pchars,
 * its start written to d_poff[pos] (and its validity to d_pvalid when given). */
int strom_bitmap_to_rows_str(const uint64_t *d_bitmap, uint64_t nwords,
                             const struct strom_filter_batch *d_batches, uint32_t nbatches,
                             int64_t *d_out, uint64_t *d_total,
                             const struct strom_qual_batch *d_strtab, uint32_t owidth,
                             int64_t *d_poff, uint8_t *d_pchars, uint8_t *d_pvalid,
                             uint64_t *d_char_cursor, void *stream);

/* A select list (csrc/kernels/colproject.hip; Arrow scans:
 * scan_where(quals, project=[...])): strom_bitmap_to_rows_proj / _str for up
 * to STROM_PROJ_MAX_COLS columns in one walk of the bitmap.  The row ids are
 * appended at *d_total, which advances by the rows appended, and every
 * column's values are written at the same positions: FIXED `width` bytes per
 * row, BOOL (Arrow LSB-first value bits) a 0/1 byte, STR32 / STR64 (offsets
 * of 4 / 8 bytes in values, the characters in aux) the row's characters
 * appended at the column's own device cursor *char_cursor in out_chars and
 * their start written to out as an int64.  out_valid, when given, gets
 * valid ? bit : 1 per selected row.  A malformed offset pair (negative,
 * decreasing, past aux_len) gives an empty string and no read outside aux.
 * Every column's table has the batches' nrows / word_base; a bit at or past
 * its batch's rows is ignored.  Nothing is written at or past the final
 * cursor positions.  `cols` is host memory, read before the call returns.
 * -22: a bad argument (ncols 0 or > STROM_PROJ_MAX_COLS, a kind or width
 * not listed, a misaligned output, two string columns on one cursor);
 * -75: more than 2^32 blocks of 256 words; -12: no scratch; 0 and nothing
 * done for nwords == 0. */
#define STROM_PROJ_MAX_COLS 16
enum { STROM_PROJ_FIXED = 1, STROM_PROJ_BOOL, STROM_PROJ_STR32, STROM_PROJ_STR64 };
struct strom_proj_col {
	int32_t  kind;
	uint32_t width;        /* FIXED: 1, 2, 4, 8 or 16 bytes */
	uint64_t table;        /* device: nbatches x strom_qual_batch of this column */
	uint64_t out;          /* FIXED/BOOL: width (BOOL: 1) bytes per selected row; STR: int64 start per row */
	uint64_t out_valid;    /* 0, or uint8 0/1 per selected row */
	uint64_t out_chars;    /* STR: the characters */
	uint64_t char_cursor;  /* STR: device uint64, advanced by the characters appended */
};
int strom_bitmap_to_rows_multi(const uint64_t *d_bitmap, uint64_t nwords,
                               const struct strom_filter_batch *d_batches, uint32_t nbatches,
                               int64_t *d_out, uint64_t *d_total,
                               const struct strom_proj_col *cols, uint32_t ncols, void *stream);
/* The same walk on the CPU, every pointer host memory (buffers of any
 * alignment): the kernel's reference and the fuzzer's target. */
int strom_bitmap_to_rows_multi_host(const uint64_t *bitmap, uint64_t nwords,
                                    const struct strom_filter_batch *batches, uint32_t nbatches,
                                    int64_t *out, uint64_t *total,
                                    const struct strom_proj_col *cols, uint32_t ncols);

/* Aggregates over the selection bitmap (csrc/kernels/colagg.hip; Arrow
 * scans: ArrowScan.aggregate): COUNT / SUM / MIN / MAX of one column's
 * selected valid rows, per key slot when a key column is given.
 *
 * One entry = one aggregated column: popcount(ops) accumulator arrays of
 * nslots 64-bit words each, in the order COUNT, SUM, MIN, MAX.  SUM holds an
 * int64/uint64 (wrapping) or, for F32/F64, a double.  MIN / MAX hold
 * order-preserving keys: signed integers x ^ 2^63, unsigned x, floats (as
 * doubles) with the sign bit set for x >= 0 and all bits flipped for x < 0;
 * NaN never enters them (MIN key > MAX key with COUNT > 0: every value was NaN).
 * type STROM_COL_NONE: only the column's validity is read (COUNT of any
 * column kind); with STROM_AGG_ALL not even that (count(*)).
 *
 * Keys: key_type one of the integer STROM_COL_* (the slot is the value, a
 * dictionary index) or STROM_COL_BOOL; slots [0, nslots - 1) are the key
 * values, slot nslots - 1 the null keys.  A selected row whose key is
 * negative or >= nslots - 1 adds one to *d_bad_keys (when given: one launch of
 * a query counts them) and nothing else.
 * d_keys == NULL: nslots must be 1.  A launch's accumulators live in LDS:
 * popcount(ops) * nslots * 8 <= STROM_AGG_LDS_BYTES, else -7.
 *
 * strom_column_agg writes one partial slab per workgroup (strom_column_agg_grid
 * of them, popcount(ops) * nslots words each) to d_slabs — no global float
 * atomics; strom_column_agg_reduce folds the slabs into the entry at d_acc in
 * a fixed order (the same geometry gives the same bits for an unkeyed float
 * sum).  strom_column_agg_init sets an entry to its identities. */
#define STROM_COL_NONE 0
#define STROM_AGG_COUNT 1
#define STROM_AGG_SUM 2
#define STROM_AGG_MIN 4
#define STROM_AGG_MAX 8
#define STROM_AGG_ALL 16       /* ignore the column's validity (count(*)) */
#define STROM_AGG_LDS_BYTES (64u << 10)
int strom_column_agg_init(uint32_t ops, uint32_t nslots, uint64_t *d_acc, void *stream);
uint32_t strom_column_agg_grid(uint64_t nwords, uint32_t ops, uint32_t nslots);
int strom_column_agg(int type, uint32_t ops, const uint64_t *d_bitmap, uint64_t nwords,
                     const struct strom_filter_batch *d_vals,
                     const struct strom_filter_batch *d_keys, int key_type, uint32_t nslots,
                     uint32_t nbatches, uint64_t *d_slabs, uint64_t slab_words,
                     uint64_t *d_bad_keys, void *stream);
int strom_column_agg_reduce(int type, uint32_t ops, uint32_t nslots, const uint64_t *d_slabs,
                            uint32_t nslabs, uint64_t *d_acc, void *stream);
/* All entries of a query over one group in one call each: launch i writes
 * e[i].slabs (sized by strom_column_agg_grid), reduce i folds them into
 * e[i].acc; malformed keys are counted by entry 0's launch only. */
struct strom_agg_entry {
	int32_t type;
	uint32_t ops;
	uint64_t vals;         /* device strom_filter_batch table of the column */
	uint64_t slabs;
	uint64_t acc;          /* the entry's words in the accumulator block */
};
int strom_column_agg_many(const struct strom_agg_entry *e, uint32_t n, const uint64_t *d_bitmap,
                          uint64_t nwords, const struct strom_filter_batch *d_keys, int key_type,
                          uint32_t nslots, uint32_t nbatches, uint64_t *d_bad_keys, void *stream);
int strom_column_agg_reduce_many(const struct strom_agg_entry *e, uint32_t n, uint32_t nslots,
                                 uint64_t nwords, void *stream);

/* Hash join of a scan's foreign-key column with a dimension table
 * (csrc/kernels/coljoin.hip; Arrow scans: the join= of ArrowScan.scan_where /
 * aggregate).
 *
 * The table is STROM_JOIN_HDR_WORDS + 2 * capacity 64-bit words on the device,
 * 16-byte aligned: the header, then capacity 16-byte slots of (key, payload in
 * the low 32 bits), open addressing with linear probing from
 * strom_join_hash(key) & (capacity - 1).  capacity is a power of two >= 2n and
 * >= 64 (strom_join_capacity).  Every int64 is a legal key: a free slot holds
 * STROM_JOIN_EMPTY, and that key itself is kept in the header.  The header's
 * MAXDISP is the largest distance of an inserted key from its home slot: a
 * probe looks at no more than MAXDISP + 1 slots.
 *
 * strom_join_build clears the table and inserts d_keys[0..n) with payload
 * d_payload[i] (NULL: i, the build row).  A key met a second time is counted
 * in DUPS and not inserted (which of the equal keys' payloads stays is not
 * defined).
 *
 * strom_column_join walks a selection bitmap like strom_column_qual (batch
 * b on words [word_base, ...), the last word bounded by nrows):
 *   SEMI  d_dst[w] = d_src[w] & match      ANTI  d_dst[w] = d_src[w] & ~match
 * over the rows that exist, where match = the row's fk is not null and is a key
 * of the table (a null fk matches nothing: ANTI keeps it).  d_dst may be d_src.
 * *d_count += popcount of the d_dst words.  type: the fk's storage, one of
 * STROM_COL_I8/I16/I32/I64/U8/U16/U32/U64 widened to int64 (a U64 value >=
 * 2^63 matches nothing); anything else is -EINVAL.  d_kout (SEMI only; may be
 * NULL): a table of the same batches whose values point to int32 buffers of
 * nrows elements; each selected matched row's payload is written at its row,
 * no other element is touched. */
#define STROM_JOIN_HDR_WORDS 8
#define STROM_JOIN_EMPTY 0x8000000000000000ull
#define STROM_JOIN_H_CAPACITY 0
#define STROM_JOIN_H_NKEYS 1
#define STROM_JOIN_H_MAXDISP 2
#define STROM_JOIN_H_DUPS 3
#define STROM_JOIN_H_HAS_EMPTY 4
#define STROM_JOIN_H_EMPTY_PAYLOAD 5
#define STROM_JOIN_SEMI 0
#define STROM_JOIN_ANTI 1
uint64_t strom_join_capacity(uint64_t n);
uint64_t strom_join_hash(int64_t key);
int strom_join_build(const int64_t *d_keys, const int32_t *d_payload, uint64_t n,
                     uint64_t *d_table, uint64_t capacity, void *stream);
int strom_column_join(int type, int how, const uint64_t *d_table, uint64_t capacity,
                      const struct strom_filter_batch *d_fk, uint32_t nbatches, uint64_t nwords,
                      const uint64_t *d_src, uint64_t *d_dst,
                      const struct strom_filter_batch *d_kout, uint64_t *d_count, void *stream);

/* A star join: 1 .. STROM_JOIN_MAX_LEGS tables applied in one walk of the
 * bitmap, in the order given (the caller puts the most selective leg first; a
 * row an earlier leg has dropped issues no load for the later ones).
 *   d_dst[w] = the rows of d_src[w] that exist and pass every leg
 * where a SEMI leg passes a row whose fk is not null and is a key of its table
 * and an ANTI leg a row whose fk is null or is not.  d_dst may be d_src (a word
 * that stays as it is is not stored); *d_count += popcount of the d_dst words.
 * Leg i reads the fk column whose batch table is d_fk[i * nbatches ..]; every
 * leg's table describes the same batches.  Per leg: `table` / `capacity` as
 * for strom_column_join, `type` the fk's storage (the eight integer types),
 * `how` SEMI or ANTI, `kout` -1 or the index of the leg's code table in d_kout
 * (table j: d_kout[j * nbatches ..], values pointing to int32 buffers of nrows
 * elements): SEMI legs only, every index below STROM_JOIN_MAX_LEGS and used by
 * one leg at most.  The leg's payload is stored for exactly the rows of the
 * d_dst word; no other element of a code buffer is touched.  -EINVAL for a
 * misaligned or NULL table, a capacity that is no power of two >= 64, another
 * type or how, kout on an ANTI leg or without d_kout, nlegs 0 or above the
 * maximum. */
#define STROM_JOIN_MAX_LEGS 4
struct strom_join_leg {
	const uint64_t *table;
	uint64_t capacity;
	uint32_t type;
	uint32_t how;
	int32_t kout;
	uint32_t reserved;
};
struct strom_join_legs {
	uint32_t nlegs;
	uint32_t reserved;
	struct strom_join_leg leg[STROM_JOIN_MAX_LEGS];
};
int strom_column_join_star(struct strom_join_legs legs,
                           const struct strom_filter_batch *d_fk, uint32_t nbatches,
                           uint64_t nwords, const uint64_t *d_src, uint64_t *d_dst,
                           const struct strom_filter_batch *d_kout, uint64_t *d_count,
                           void *stream);

/* Hash GROUP BY on an integer key column (csrc/kernels/colgroup.hip; Arrow
 * scans: by=HashBy(col) of ArrowScan.aggregate) for key domains that do not
 * fit strom_column_agg's LDS.
 *
 * The table is STROM_GROUP_HDR_WORDS + capacity 64-bit words on the device:
 * the header, then one key word per slot, open addressing with linear probing
 * from strom_join_hash(key) & (capacity - 1).  capacity is a power of two
 * >= 2 * groups (strom_group_capacity), at most STROM_GROUP_MAX_CAPACITY.  A
 * key is the 64-bit pattern of the column's value (signed types sign-extended,
 * unsigned ones zero-extended).  A free slot holds STROM_JOIN_EMPTY; the key
 * with that pattern is legal and has the reserved code capacity + 1, the null
 * keys have code capacity.  Header: NKEYS the distinct non-null keys that got
 * a code, OVERFLOW the selected rows that found no slot, HAS_EMPTY whether the
 * key STROM_JOIN_EMPTY was met.
 *
 * Accumulators: per entry popcount(ops) arrays of capacity + 2 words in the
 * order and encoding of strom_column_agg, indexed by code.  strom_group_init
 * clears the table and sets the arrays at e[i].acc to their identities
 * (e[i].type, vals and slabs are not read); nothing else ever writes a word
 * of either without an atomic.
 *
 * strom_group_codes walks a selection bitmap like strom_column_join: each
 * selected row that exists finds or inserts its key and gets its int32 code
 * written at its row of d_codes (a table of the same batches whose values
 * point to int32 buffers of nrows elements).  d_dst[w] = d_src[w] over the rows
 * that exist, minus the rows that found no slot (their code is written as 0);
 * d_dst may be d_src.  type as for strom_column_join, U64 over its whole range.
 * Launches on different streams may share a table.
 *
 * strom_group_agg adds one entry's column over the bitmap into the arrays at
 * d_acc with device-scope atomics (no slabs, no reduce: float sums depend on
 * arrival order); a code outside [0, capacity + 2) is not followed.  combine
 * != 0: in a word of mixed codes the rows that share the first selected row's
 * code (when there are two or more) stay in the wave's registers, as a word of
 * one code does, and are added when that code changes.
 *
 * Composite keys (GROUP BY a, b, ...: by=HashBy([a, b]) of ArrowScan.aggregate):
 * strom_group_codes_multi packs up to STROM_GROUP_MAX_KEYS components into the
 * one key word and walks the same table.  Component i has a field of `bits`
 * value bits (1 .. its storage width) at bit `shift`, one bit wider when
 * `nullable`; the first component's field is the topmost, the fields do not
 * overlap and bits of the word that no field covers are zero.  A signed value
 * is stored as v + 2^(bits - 1), an unsigned one as it is, a null as the
 * field's top bit alone: unsigned order of the word is lexicographic order of
 * the tuples, each column ascending, nulls after all values.  A row with a
 * value that does not fit its `bits` (or a null in a component not declared
 * nullable) is cleared from d_dst, has code 0 written and is counted once, in
 * header word STROM_GROUP_H_RANGE + i of its first such component i.  The word
 * STROM_JOIN_EMPTY is a legal key here as well (code capacity + 1, HAS_EMPTY);
 * the null code `capacity` is never written.  d_keys holds the components'
 * batch tables back to back (component i: d_keys[i * nbatches ..]), all of the
 * same batches; a component's values may be the int32 buffers of d_codes
 * themselves (a row's components are read before its code is stored).
 * Everything else as strom_group_codes, which it leaves alone. */
#define STROM_GROUP_HDR_WORDS 8
#define STROM_GROUP_MAX_CAPACITY (1ull << 25)
#define STROM_GROUP_H_CAPACITY 0
#define STROM_GROUP_H_NKEYS 1
#define STROM_GROUP_H_OVERFLOW 2
#define STROM_GROUP_H_HAS_EMPTY 3
#define STROM_GROUP_H_RANGE 4           /* words 4 .. 7: one per component */
#define STROM_GROUP_MAX_KEYS 4
struct strom_group_key {
  uint32_t type;                /* STROM_COL_I8 .. U64: how the values are stored */
  uint32_t bits;                /* value bits of the field */
  uint32_t shift;               /* the field's lowest bit in the key word */
  uint32_t nullable;            /* 1: one more bit on top, set for a null */
};
struct strom_group_keys {
  uint32_t nkeys;
  uint32_t reserved;
  struct strom_group_key k[STROM_GROUP_MAX_KEYS];
};
uint64_t strom_group_capacity(uint64_t groups);
int strom_group_init(uint64_t *d_table, uint64_t capacity, const struct strom_agg_entry *e,
                     uint32_t n, void *stream);
int strom_group_codes(int type, uint64_t *d_table, uint64_t capacity,
                      const struct strom_filter_batch *d_keys, uint32_t nbatches, uint64_t nwords,
                      const uint64_t *d_src, uint64_t *d_dst,
                      const struct strom_filter_batch *d_codes, void *stream);
int strom_group_codes_multi(struct strom_group_keys keys, uint64_t *d_table, uint64_t capacity,
                            const struct strom_filter_batch *d_keys, uint32_t nbatches,
                            uint64_t nwords, const uint64_t *d_src, uint64_t *d_dst,
                            const struct strom_filter_batch *d_codes, void *stream);
int strom_group_agg(int type, uint32_t ops, const uint64_t *d_bitmap, uint64_t nwords,
                    const struct strom_filter_batch *d_vals,
                    const struct strom_filter_batch *d_codes, uint32_t nbatches, uint64_t *d_acc,
                    uint64_t capacity, int combine, void *stream);
int strom_group_agg_many(const struct strom_agg_entry *e, uint32_t n, const uint64_t *d_bitmap,
                         uint64_t nwords, const struct strom_filter_batch *d_codes,
                         uint32_t nbatches, uint64_t capacity, int combine, void *stream);

/* ORDER BY one column LIMIT k over the selection bitmap
 * (csrc/kernels/coltopk.hip; Arrow scans: ArrowScan.top).
 *
 * Order: (class, key, row), all ascending.  class 0 a value, 1 a NaN, 2 a
 * null — in both directions.  key: the MIN / MAX encoding of
 * strom_column_agg (signed x ^ 2^63, unsigned x, floats as doubles with the
 * sign bit set for x >= 0 and all bits flipped for x < 0, -0.0 taken as
 * +0.0), every bit inverted with STROM_TOPK_DESC; 0 for a NaN or a null.
 * row: the file-global row id (row_base + local row), so the order is total
 * and equal values come back in file order whatever the direction.
 *
 * A candidate is STROM_TOPK_ENTRY_WORDS 64-bit words:
 *   word 0  key
 *   word 1  meta = class << 62 | row << 2 | negzero << 1 | pvalid
 *           (negzero: the value was -0.0; pvalid: the payload is not null;
 *           rows are < 2^60)
 *   word 2  payload: the carried column's value of the row, zero-extended
 *           from pay_width bytes; 0 when it is null or nothing is carried
 * so a < b is (a.meta >> 62, a.key, a.meta) < (b.meta >> 62, b.key, b.meta).
 *
 * State: STROM_TOPK_HDR_WORDS + 3 * k words on the device
 * (strom_topk_state_words).  Header: K the k it was initialised for, COUNT
 * the candidates held (<= k), SEEN the selected rows of every group merged
 * so far, THRESH the threshold key, ERRORS the slabs and states refused (a
 * count above k, another k: nothing of them is followed), MERGES the merges
 * done; words 6, 7 are zero.  Then COUNT candidates, sorted; the words behind
 * them are never written.  THRESH is the key of the k-th candidate once k are
 * held and that candidate is a value, else ~0 ("everything passes"): a row
 * may enter the result only if THRESH is ~0 or it is a value with key <=
 * THRESH.  THRESH only ever decreases.  Only strom_topk_init and
 * strom_topk_merge write a state.
 *
 * strom_column_topk walks the bitmap like strom_column_join (batch b on
 * words [word_base, ...), the last word bounded by nrows; a null of d_vals is
 * class 2) with strom_column_topk_grid(nwords, k) workgroups, workgroup g
 * taking words 4 * g + 4 * grid * t + (0 .. 3), and leaves one slab per
 * workgroup at d_slabs + g * strom_topk_slab_words(k):
 *   word 0  n, the candidates that follow (<= k)
 *   word 1  the selected rows the workgroup walked
 *   then n candidates, sorted: the workgroup's k best among its rows that
 *   passed THRESH as it was when the workgroup read it (one 64-bit load; the
 *   words behind them are not written).
 * THRESH may be stored by a merge on another stream meanwhile: an older
 * value passes more rows, never fewer, and every row it rejects is behind k
 * rows the state already holds.  d_pay (may be NULL): a table of the same
 * batches for the carried column, pay_width 1, 2, 4 or 8 bytes per row — the
 * slot's int32 code buffers are such a table.  type: STROM_COL_I8 .. U64,
 * F32, F64.  The grid keeps grid * k <= 2^18 candidates of slabs.
 *
 * strom_topk_merge (one workgroup; the scan runs it in group order on its
 * emit stream) folds nslabs slabs and the state's candidates into the
 * state's k best and stores SEEN, COUNT and the new THRESH.
 *
 * STROM_TOPK_MAX_K: a workgroup collects candidates in an LDS buffer of C
 * entries of 24 bytes and sorts it (bitonic, over the entries held: the
 * network needs no power of two of storage) and cuts it to k whenever more
 * than C - 256 are held — 256 lanes append between two looks at the fill.
 * C = max(2k, 64) + 256, at most STROM_TOPK_MAX_K + 256, so C >= k + 256
 * always.  The CU's LDS is 160 KiB = 163,840 bytes, of which the kernels keep
 * some 64 bytes besides the buffer: 24 C <= 163,776 allows C = 6,824, k =
 * 6,568; the limit is the multiple of 1,024 below, a buffer of 150 KiB.
 *
 * The strom_topk_host_* functions are the same phases on the CPU over host
 * pointers, workgroup by workgroup (csrc/tests/coltopk_fuzz.cc runs them
 * under ASan + UBSan). */
#define STROM_TOPK_MAX_K 6144
#define STROM_TOPK_HDR_WORDS 8
#define STROM_TOPK_ENTRY_WORDS 3
#define STROM_TOPK_SLAB_HDR_WORDS 2
#define STROM_TOPK_H_K 0
#define STROM_TOPK_H_COUNT 1
#define STROM_TOPK_H_SEEN 2
#define STROM_TOPK_H_THRESH 3
#define STROM_TOPK_H_ERRORS 4
#define STROM_TOPK_H_MERGES 5
#define STROM_TOPK_DESC 1
uint64_t strom_topk_state_words(uint32_t k);
uint64_t strom_topk_slab_words(uint32_t k);
uint32_t strom_column_topk_grid(uint64_t nwords, uint32_t k);
int strom_topk_init(uint64_t *d_state, uint32_t k, void *stream);
int strom_column_topk(int type, uint32_t flags, uint32_t k, const uint64_t *d_bitmap,
                      uint64_t nwords, const struct strom_filter_batch *d_vals,
                      const struct strom_filter_batch *d_pay, uint32_t pay_width,
                      uint32_t nbatches, const uint64_t *d_state, uint64_t *d_slabs,
                      void *stream);
int strom_topk_merge(uint32_t k, const uint64_t *d_slabs, uint32_t nslabs, uint64_t *d_state,
                     void *stream);
int strom_topk_host_init(uint64_t *state, uint32_t k);
int strom_topk_host_select(int type, uint32_t flags, uint32_t k, const uint64_t *bitmap,
                           uint64_t nwords, const struct strom_filter_batch *vals,
                           const struct strom_filter_batch *pay, uint32_t pay_width,
                           uint32_t nbatches, const uint64_t *state, uint64_t *slabs);
int strom_topk_host_merge(uint32_t k, const uint64_t *slabs, uint32_t nslabs, uint64_t *state);

/* ORDER BY on several columns (csrc/kernels/colsort.hip; Arrow scans:
 * scan_where(quals, project=[...], order_by=[...], limit=, offset=)): a stable
 * LSD radix sort over the n selected rows a select list's emit left in HBM —
 * per column its values and, when it may hold nulls, one validity byte (0/1)
 * per row.  The order is strom_column_topk's: a value before a NaN before a
 * null in both directions, -0.0 equal to +0.0, equal keys in the order they
 * came in.
 *
 * All state is the caller's: two uint64 key arrays and two uint32 permutation
 * arrays of n entries each (24 bytes per row) and a work table of
 * strom_sort_work_bytes(n) bytes: 256 uint32 counts per tile of
 * STROM_SORT_TILE keys, digit-major, and 256 digit totals behind them.
 * n < 2^32.
 *
 * strom_sort_encode writes key[i] = the key of values[perm[i]]: the value at
 * the storage type's own width (type: STROM_COL_I8 .. U64, F32, F64) — sign
 * bit flipped for signed integers, the monotone float map with -0.0 folded
 * into +0.0, every bit of the width inverted with STROM_SORT_DESC, 0 for a
 * NaN or a null (valid, may be NULL: no nulls).  With STROM_SORT_CLASS the
 * key is the class instead: 0 a value, 1 a NaN, 2 a null.  With
 * STROM_SORT_FIRST perm is written (perm[i] = i), not read.  A permutation
 * entry >= n gives key 0.  A column is sorted by one strom_sort_pass per byte
 * of its storage type, shift = 0, 8, ..., and where it is a float type or has
 * nulls by a CLASS encode and one more pass at shift 0; the columns go from
 * the least significant to the most.
 *
 * strom_sort_pass: one stable 8-bit pass (key_in, perm_in) -> (key_out,
 * perm_out) by the digit at `shift` (a multiple of 8 up to 56): a histogram
 * launch (one workgroup per tile, its counts into its own column of the
 * table, no global atomics), a scan launch (workgroup d turns row d into
 * exclusive prefixes, STROM_SORT_SCAN_THREADS entries a trip, and stores the
 * row's total) and a scatter launch.  No workgroup waits for another.
 *
 * strom_sort_apply: out[i] = in[perm[first + i]] for i < count (first and
 * count are cut to n) for the row ids (d_rows_in / d_rows_out, both or
 * neither) and up to STROM_SORT_MAX_COLS columns in one launch; `cols` is
 * host memory.  STROM_SORT_FIXED: `width` bytes per row (1, 2, 4, 8 or 16);
 * STROM_SORT_LEN: `in` the int64 starts of a string column (n + 1 of them),
 * `out` receives the row's length as int64.  out_valid (0: none) receives
 * in_valid's byte (in_valid 0: 1).  A permutation entry >= n writes zeros and
 * adds one to *d_err; nothing is read out of bounds.
 *
 * strom_sort_chars copies a string column's characters in output order:
 * d_out_off the count + 1 int64 output offsets (the exclusive prefix of
 * strom_sort_apply's lengths), in_len the bytes of d_in_chars, out_cap those
 * of d_out_chars (4-byte aligned for whole-dword stores).
 *
 * Every entry returns -22 and launches nothing for a null pointer, n >= 2^32,
 * an unknown type, flag, kind or width, more than STROM_SORT_MAX_COLS
 * columns; n = 0 (or an empty window) returns 0 without a launch.  The
 * strom_sort_*_host functions are the same steps on the CPU over host
 * pointers (csrc/tests/colsort_fuzz.cc runs them under ASan + UBSan). */
#define STROM_SORT_TILE 4096
#define STROM_SORT_SCAN_THREADS 256
#define STROM_SORT_MAX_COLS 16
#define STROM_SORT_DESC 1
#define STROM_SORT_CLASS 2
#define STROM_SORT_FIRST 4
enum { STROM_SORT_FIXED = 1, STROM_SORT_LEN = 2 };
struct strom_sort_col {
  uint32_t kind;
  uint32_t width;
  uint64_t in;
  uint64_t out;
  uint64_t in_valid;
  uint64_t out_valid;
};
uint64_t strom_sort_work_bytes(uint64_t n);
int strom_sort_encode(int type, uint32_t flags, const void *d_values, const uint8_t *d_valid,
                      uint32_t *d_perm, uint64_t n, uint64_t *d_key, void *stream);
int strom_sort_pass(const uint64_t *d_key_in, const uint32_t *d_perm_in, uint64_t *d_key_out,
                    uint32_t *d_perm_out, uint64_t n, uint32_t shift, uint32_t *d_work,
                    void *stream);
int strom_sort_apply(const uint32_t *d_perm, uint64_t n, uint64_t first, uint64_t count,
                     const int64_t *d_rows_in, int64_t *d_rows_out,
                     const struct strom_sort_col *cols, uint32_t ncols, uint64_t *d_err,
                     void *stream);
int strom_sort_chars(const uint32_t *d_perm, uint64_t n, uint64_t first, uint64_t count,
                     const int64_t *d_in_off, const uint8_t *d_in_chars, uint64_t in_len,
                     const int64_t *d_out_off, uint8_t *d_out_chars, uint64_t out_cap,
                     void *stream);
int strom_sort_encode_host(int type, uint32_t flags, const void *values, const uint8_t *valid,
                           uint32_t *perm, uint64_t n, uint64_t *key);
int strom_sort_pass_host(const uint64_t *key_in, const uint32_t *perm_in, uint64_t *key_out,
                         uint32_t *perm_out, uint64_t n, uint32_t shift, uint32_t *work);
int strom_sort_apply_host(const uint32_t *perm, uint64_t n, uint64_t first, uint64_t count,
                          const int64_t *rows_in, int64_t *rows_out,
                          const struct strom_sort_col *cols, uint32_t ncols, uint64_t *err);
int strom_sort_chars_host(const uint32_t *perm, uint64_t n, uint64_t first, uint64_t count,
                          const int64_t *in_off, const uint8_t *in_chars, uint64_t in_len,
                          const int64_t *out_off, uint8_t *out_chars, uint64_t out_cap);

/* Computed columns (csrc/kernels/colexpr.hip; Arrow scans: an E expression
 * where a column name is accepted; nvme_strom_amd/ops/colexpr.py compiles
 * them): one arithmetic expression over up to STROM_EXPR_MAX_COLS source
 * columns, evaluated for every row of a group's batches in one launch into an
 * 8-byte column that the qualifier, aggregate, group, top-k and emit kernels
 * read like a stored one (STROM_COL_I64 or STROM_COL_F64).
 *
 * The program is a postfix list of at most STROM_EXPR_MAX_OPS ops over a
 * stack of at most STROM_EXPR_MAX_DEPTH values, all of one domain:
 *   STROM_EXPR_INT  sources I8 .. I64, U8 .. U32 sign-/zero-extended to int64;
 *                   ADD SUB MUL NEG ABS wrap in 64 bits (NEG and ABS of
 *                   INT64_MIN are INT64_MIN); FDIV and MOD by the immediate
 *                   (> 0) round toward minus infinity, MOD within [0, imm).
 *   STROM_EXPR_FLT  integer sources converted with (double), F32 widened; ADD
 *                   SUB MUL DIV are IEEE double operations, each rounded on
 *                   its own (never fused); NEG and ABS act on the sign bit.  A
 *                   NaN result is stored as 0x7ff8000000000000.
 * COL pushes source column arg, CONST the immediate (an int64, or the bits
 * of a double).  F32 / F64 sources and DIV need the FLT domain, FDIV and MOD
 * the INT domain.
 *
 * d_src holds ncols tables of nbatches entries (column c's at d_src + c *
 * nbatches), all of the same batches; d_out is one more table of them whose
 * values receive row i's result at ((uint64_t *)values)[i] and whose valid
 * (never 0) receives whole validity words, word k of the batch at
 * ((uint64_t *)valid)[k]: the AND of the sources' validity words (valid = 0:
 * all ones), the batch's last word cut to nrows.  Only rows whose validity
 * bit is set are loaded and stored.  d_sel (may be NULL) is a selection
 * bitmap of nwords words: a word whose d_sel word is 0 is not evaluated, its
 * validity word is stored as 0 and no value of it is stored.
 *
 * strom_expr_check: 0, or -22 for an unknown opcode or domain, no op or more
 * than STROM_EXPR_MAX_OPS, more than STROM_EXPR_MAX_COLS columns, a column
 * index >= ncols, a source type the domain does not take, an op of the other
 * domain, an immediate divisor <= 0, a stack underflow, a depth above
 * STROM_EXPR_MAX_DEPTH or a final depth other than 1.  strom_column_expr
 * runs it first and launches nothing unless it passes.
 * strom_column_expr_host is the same walk on the CPU over host pointers
 * (csrc/tests/colexpr_fuzz.cc runs it under ASan + UBSan). */
#define STROM_EXPR_MAX_OPS 16
#define STROM_EXPR_MAX_COLS 4
#define STROM_EXPR_MAX_DEPTH 8
#define STROM_EXPR_INT 0
#define STROM_EXPR_FLT 1
#define STROM_XOP_COL 1
#define STROM_XOP_CONST 2
#define STROM_XOP_ADD 3
#define STROM_XOP_SUB 4
#define STROM_XOP_MUL 5
#define STROM_XOP_NEG 6
#define STROM_XOP_ABS 7
#define STROM_XOP_DIV 8
#define STROM_XOP_FDIV 9
#define STROM_XOP_MOD 10
struct strom_expr_op {
	uint32_t op;
	uint32_t arg;          /* COL: the source column */
	uint64_t imm;          /* CONST, FDIV, MOD */
};
struct strom_expr {
	uint32_t domain;
	uint32_t nops;
	uint32_t ncols;
	uint32_t reserved;
	uint32_t col_type[STROM_EXPR_MAX_COLS];
	struct strom_expr_op ops[STROM_EXPR_MAX_OPS];
};
int strom_expr_check(const struct strom_expr *e);
int strom_column_expr(const struct strom_expr *e, const struct strom_filter_batch *d_src,
                      uint32_t nbatches, uint64_t nwords, const uint64_t *d_sel,
                      const struct strom_filter_batch *d_out, void *stream);
int strom_column_expr_host(const struct strom_expr *e, const struct strom_filter_batch *src,
                           uint32_t nbatches, uint64_t nwords, const uint64_t *sel,
                           const struct strom_filter_batch *out);

#ifdef __cplusplus
}
#endif
#endif /* STROM_STROM_H */
