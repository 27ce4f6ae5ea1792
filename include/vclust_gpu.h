/*
 * vclust_gpu.h — C ABI of libvclust_gpu.so, the MI355X-native replacement of the two native
 * tools on Vclust's prefilter -> align hot path.
 *
 * The reference has no library ABI for this path: vclust.py drives `bin/kmer-db` and
 * `bin/lz-ani` through subprocess.run() (vclust.py:762-807).  Every entry point below
 * names the process invocation it replaces:
 *
 *   vg_prefilter      <- kmer-db build (vclust.py:953-964) + all2all-sp/-parts
 *                        (vclust.py:1005-1017) + distance ani-shorter (vclust.py:1045-1055),
 *                        i.e. the whole body of handle_prefilter (vclust.py:1433-1471)
 *   vg_align          <- lz-ani all2all (vclust.py:1142-1181, run at vclust.py:1521)
 *   vg_cluster        <- clusty (cmd_clusty, vclust.py:1184-1278, run at vclust.py:1557) for single, cd-hit,
 *                        uclust and set-cover
 *   vg_deduplicate    <- mfasta-tool mrds (cmd_mfasta_deduplicate, vclust.py:810-866, run at vclust.py:1351)
 *   vg_version        <- `kmer-db -version` / `lz-ani --version` (vclust.py:1323-1331)
 *
 * The finer-grained functions (genome sets, integer kernels, writers) are what the two
 * calls above are made of; they are exported so that (a) the Python front-end can shard the
 * integer work over one process per GPU and gather rows with torch.distributed (RCCL), and
 * (b) the parity tests can compare integers with the CPU oracle.
 *
 * Conventions: every function returns 0 on success and a negative code on error;
 * vg_last_error() returns a thread-local, library-owned, NUL-terminated message.  Calls
 * block.  Paths are UTF-8, owned by the caller.  Arrays returned through `T** out` are
 * owned by the library and released with vg_free().  No C++ exceptions cross the ABI.
 * There is NO CPU fallback: without a HIP device every compute call fails with VG_ENODEV.
 * One process drives one GPU: the library keeps one device, one pair of queues and one workspace cache per process, and
 * its compute entry points are to be called by one thread at a time (they use many threads and the whole GPU themselves).
 */
#ifndef VCLUST_GPU_H
#define VCLUST_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    VG_OK = 0, VG_EINVAL = -1, VG_EIO = -2, VG_ENODEV = -3, VG_EHIP = -4, VG_ENOMEM = -5,
    VG_EOVERFLOW = -6
};

const char* vg_version(void);
const char* vg_last_error(void);
void        vg_free(void* p);
/* number of visible HIP devices (0 when there is none); selects the device used by this
 * process for all later calls (one process per GPU) */
int vg_device_count(void);
int vg_set_device(int device);
/* the library keeps released device blocks in a cache (no hipMalloc on the hot path); this returns them to
 * the driver, e.g. before another process needs the HBM -- together with the reference indexes a vg_lz_prepare
 * may have left behind (that plan is process-global: one per process, replaced by the next vg_lz_prepare / vg_lz_align) */
void vg_release_device_memory(void);
/* allocator self-test (no reference call site): `cycles` rounds of allocating blocks of the given byte sizes through the
 * library's device allocator, writing and reading back a pattern at both ends of each, releasing them and returning the
 * cache to the driver */
int vg_alloc_selftest(const int64_t* sizes, int n_sizes, int cycles);
/* blocking copy between host memory and memory of the current device (for vg_comm callbacks that stage through the host) */
int vg_copy(void* dst, const void* src, int64_t bytes, int to_host);

/* ------------------------------------------------------------------ genome sets ------- */
typedef struct vg_genomes vg_genomes;

/* FASTA / FASTA.gz ingest.  n_paths == 1 && multisample: one genome per record
 * (`-multisample-fasta`, vclust.py:962-963 / `--multisample-fasta true`, :1159-1160);
 * otherwise one genome per file, records joined by one N (vclust.py:692-700).
 * Genome name = first header token (multisample) or file name (directory mode). */
int vg_genomes_load(const char* const* paths, int n_paths, int multisample, int n_threads,
                    vg_genomes** out);
/* A database and new genomes as ONE set: the genomes of db_paths, then those of new_paths; *n_db_genomes receives the number of
 * database genomes (ids 0 .. n_db - 1; the new ones are n_db .. n - 1).  The set is what vg_genomes_load would make of the
 * concatenated input.  multisample: exactly one file on each side, one genome per record, the records of the database file first
 * (any other count is VG_EINVAL); otherwise one genome per file.  A name that occurs on both sides is VG_EINVAL naming it (the
 * filter reader maps names to ids), and so is a combined set of fewer than two genomes; both are raised before anything is packed.  Stands in for the input of `kmer-db new2all`; vclust.py has
 * no call site for it. */
int vg_genomes_load_db_new(const char* const* db_paths, int n_db, const char* const* new_paths, int n_new, int multisample,
                           int n_threads, vg_genomes** out, int* n_db_genomes);
/* synthetic / in-memory input: codes 0..3 = ACGT, >3 = N; genome g = codes[offsets[g] ..
 * offsets[g+1]); names may be NULL ("g<idx>") */
int vg_genomes_from_codes(const uint8_t* codes, const int64_t* offsets, int n_genomes,
                          const char* const* names, vg_genomes** out);
void        vg_genomes_free(vg_genomes* g);
int         vg_genomes_count(const vg_genomes* g);
int64_t     vg_genomes_total_len(const vg_genomes* g);
int         vg_genomes_lengths(const vg_genomes* g, int64_t* out /* n */);
const char* vg_genomes_name(const vg_genomes* g, int idx);
/* the bases of genome idx as the set holds them on the host (codes 0..3 = ACGT, 4 = N), out = len[idx] bytes:
 * the inverse of the packing, for checks of the reader (no reference call site) */
int         vg_genomes_codes(const vg_genomes* g, int idx, uint8_t* out);
/* 2-bit packed bases + N mask -> HBM of the current device (idempotent); the kernels' own copy of the bases -- bit planes,
 * DESIGN.md section 3 -- is made from them on the device at the first prefilter / align call */
int vg_genomes_to_device(vg_genomes* g);
/* A subset of a resident set (this repository's call; no reference call site): *out is a new set holding the genomes ids[0 .. n_ids)
 * of g, in that order, with their names, lengths and part counts.  It is built on the device from g's resident 2-bit codes and N mask
 * by one gather kernel (profile scope `derep_subset`); no base travels from the host.  The subset keeps g's block size, lays its
 * genomes out by the loader's padding rule (at least one masked padding base behind every genome) and is resident on g's device; g is
 * not changed and need not outlive it.  Its host copy of the bases stays empty: vg_genomes_codes downloads the genome it is asked
 * for, and the sharded entry points (vg_kmer_shared_sharded, vg_lz_align_sharded, vg_lz_align_pairs_sharded) refuse such a set with
 * VG_EINVAL.  An id outside [0, n) or listed twice is VG_EINVAL naming it, and so is a set that is not resident
 * (vg_genomes_to_device); all three are raised before any device use.  n_ids = 0 gives a valid empty set. */
int vg_genomes_subset(const vg_genomes* g, const int32_t* ids, int n_ids, vg_genomes** out);
/* A subset extended in place (this repository's call; no reference call site): the genomes ids[0 .. n_ids) of `parent` are appended
 * behind the last genome of `sub`, in that order, by the layout rules of vg_genomes_subset and by one gather kernel (profile scope
 * `derep_extend`) that writes the appended genomes and the slack behind them and neither reads nor copies the genomes already there.
 * sub must be a set vg_genomes_subset made from this very parent (it may be empty); afterwards it is, to every kernel, the set
 * vg_genomes_subset would make of all its genomes.  When the appended bases do not fit, the buffers grow to at least 1.5 times their
 * size, which costs one copy device to device of the resident part (vg_genomes_reserve avoids it).  Everything the set keeps of its
 * contents (bit planes, align order, the index plans of vg_lz_prepare) is dropped and remade lazily.  VG_EINVAL, before any device
 * use: a null argument, an id outside the parent, listed twice or in sub already, a sub that vg_genomes_subset did not make or made
 * from another parent, a parent that is not resident or on another device than sub.  n_ids = 0 is valid. */
int vg_genomes_extend(vg_genomes* sub, const vg_genomes* parent, const int32_t* ids, int n_ids);
/* The inverse: every genome of `sub` from n_keep on is dropped, and the slack behind the new last genome is written afresh, so that
 * a kernel that reads past the end sees what it sees in the set vg_genomes_subset makes of the kept genomes.  The capacity stays;
 * the caches are dropped as by vg_genomes_extend.  VG_EINVAL, before any device use: null, n_keep outside 0..n, a set that
 * vg_genomes_subset did not make. */
int vg_genomes_truncate(vg_genomes* sub, int n_keep);
/* Room for `genomes` genomes of `bases` bases in all (padding is added by the call: a whole block per genome, the worst case of the
 * loader's rule), so that extending `sub` up to there never moves it.  Never shrinks.  VG_EINVAL, before any device use: null, a
 * negative count, a set that vg_genomes_subset did not make. */
int vg_genomes_reserve(vg_genomes* sub, int64_t bases, int64_t genomes);

/* ------------------------------------------------------------------ prefilter --------- */
typedef struct { uint32_t a, b, shared; } vg_pair_count;   /* a > b (input order ids) */

/* Integer core of the prefilter on the GPU: per-genome distinct canonical k-mer counts and
 * the sparse all-vs-all shared-k-mer counts (K1+K2 of SURVEY §8a).
 *   fraction        --kmers-fraction (vclust.py:241-248); 1.0 = all k-mers
 *   shard/n_shards  k-mer range handled by this call -- a range of the scrambled key's top bits for sets below 2^32 bases
 *                   without a fraction, a hash of its low bits otherwise -- (multi-GPU: one shard per rank;
 *                   set sizes and shared counts of the shards ADD UP)
 *   min_shared      pairs with fewer shared k-mers are not emitted (use 1 when n_shards>1)
 * set_sizes: n entries.  pairs: unordered; released with vg_free(). */
int vg_kmer_shared(vg_genomes* g, int k, double fraction, int shard, int n_shards,
                   uint32_t min_shared, int64_t* set_sizes, vg_pair_count** pairs,
                   int64_t* n_pairs);
/* New genomes against a database (`kmer-db new2all`; vclust.py never exposed it, so there is no call site).  The set is the
 * database genomes 0 .. n_db - 1 followed by the new genomes n_db .. n - 1 (vg_genomes_load_db_new, or any set and any n_db).
 * pairs: the result of vg_kmer_shared(g, k, fraction, 0, 1, min_shared, ...) restricted to the pairs (a, b), a > b, with
 * a >= n_db -- every pair that contains a new genome, same counts.  n_db = 0 is that call's result; n_db = n gives no pair.
 * set_sizes (n entries): exact for every new genome and for every database genome that occurs in a returned pair, -1 for the other
 * database genomes.  vg_filter_pairs and vg_write_fltr read the sizes of the two genomes of a pair and no others, so they take
 * these arrays as they are; vg_write_fltr then writes the all-vs-all file of the set with the database rows empty.
 * One device.  n_db < 0 or n_db > n is VG_EINVAL, raised before any device use.
 * Two routes, same result: the passes of vg_kmer_shared (every option, sub-shards included) with the SpGEMM
 * launched over the new genomes' rows only; and, for a dense single pass (no fraction, no sub-shards, below 2^32 padded positions)
 * that the bucket pipeline accepts, the masked route, which indexes only the k-mers a new genome can share (profile scope
 * `kmer_new_mask`) and restores the sizes of the database genomes in pairs by a second masked pass (`kmer_new_sizes`). */
int vg_kmer_shared_new(vg_genomes* g, int n_db, int k, double fraction, uint32_t min_shared, int64_t* set_sizes,
                       vg_pair_count** pairs, int64_t* n_pairs);
/* route of vg_kmer_shared_new: 0 (default) = automatic, 1 = never the masked route, 2 = the masked route wherever it applies (tests,
 * tools/new2all_timing.py); no reference call site */
void vg_set_new_path(int mode);
/* Which index geometry a call will take (tests and tooling; no reference call site).  Host only: no device is needed or touched.
 * vg_kmer_geometry reports what the bucket pipeline decides for the FIRST pass of vg_kmer_shared(g, k, fraction, shard, n_shards,
 * ...), by calling the function that pass calls; vg_set_subshards and the developer switches apply to it as they do to the pass.
 * vg_kmer_geometry_at is the same question for the dense single pass (no fraction, one shard, no sub-shards) over a set of
 * `padded_positions` positions, without a set: the pass of vg_kmer_shared(g, k, 1.0, 0, 1, ...) and the level 1 of the masked
 * route of vg_kmer_shared_new.
 *   accepted    1 = the bucket pipeline takes the pass; 0 = it declines (the general path); -1 = the pass has a compact source
 *               (a fraction, HASH shards): its geometry follows from the number of kept k-mers, which only the device knows.
 *               Only P and n_passes are filled unless accepted == 1.
 *   P           padded positions of the set;  n_passes: passes the call is cut into (1 = no sub-shards)
 *   levels      partition levels (1 or 2);  total_bits = B1 + B2: key bits the two levels partition on
 *   st_tiles    8 192-position tiles per level-1 super-tile;  n_st: super-tiles of the pass
 *   u_st        super-tiles per level-2 unit
 *   g_st        short records only: super-tiles per 2^25-position group where a unit spans several groups (u_st / g_st of them),
 *               0 where a unit lies inside one group
 *   tile32k     level 1 scatters whole 32 768-position tiles;  narrow: level-2 records carry one key word
 *   short_rec   level-1 records are 8 bytes (key bits, position modulo 2^25) instead of 12
 * vg_kmer_level2_slots answers, for the same pass and by the same function, how its level 2 runs: *slots > 0 = in one pass, without
 * a count, every final bucket owning that many record slots; 0 = the counted level 2 (RANGE and HASH shards, sub-shards, one
 * level, the wide scatter, fewer than 256 level-1 buckets) or a pass the bucket pipeline does not take as a dense one. */
typedef struct {
    int accepted; int64_t P; int n_passes;
    int levels, total_bits, B1, B2;
    int st_tiles; int64_t n_st; int u_st, g_st;
    int tile32k, narrow, short_rec;
} vg_kmer_geometry_info;
int vg_kmer_geometry(const vg_genomes* g, int k, double fraction, int shard, int n_shards, vg_kmer_geometry_info* info);
int vg_kmer_level2_slots(const vg_genomes* g, int k, double fraction, int shard, int n_shards, int* slots);
int vg_kmer_geometry_at(int64_t padded_positions, int k, vg_kmer_geometry_info* info);
/* The row-pointer rule of a prefilter pass (tests and tooling; no reference call site).  Host only: no device is needed or touched.
 * A pass whose genome list holds `entries` slots over `n_genomes` genomes writes the row pointer of a k-mer with ONE smaller partner as
 * 0xFFFFFFFF - partner where entries + n_genomes < 2^32; *inline_lo = 2^32 - n_genomes is then the smallest such value.  0 = the pass
 * inlines nothing (no room beside the plain values 1 .. entries, or the developer switch VG_ROWPTR_INLINE=0). */
int vg_rowptr_inline_lo(int64_t entries, int64_t n_genomes, uint32_t* inline_lo);
/* distinct canonical k-mers of one genome, ascending (parity tests) */
int vg_kmer_set(vg_genomes* g, int idx, int k, double fraction, uint64_t** out, int64_t* n_out);

/* K3+K4: ani-shorter transform, thresholds, fltr.txt (example/output/fltr.txt layout).
 * Sums duplicate (a,b) entries first, so concatenated per-shard outputs are accepted. */
int vg_write_fltr(const vg_genomes* g, int k, double fraction, int min_kmers, double min_ident,
                  int max_seqs, const int64_t* set_sizes, const vg_pair_count* pairs,
                  int64_t n_pairs, const char* out_path);

/* K3 without the file: the pairs that vg_write_fltr would print (shared >= min_kmers and
 * ani-shorter >= min_ident, same arithmetic), for a prefilter -> align hand-over in memory.
 * One entry per pair expected (vg_kmer_shared output, or merged shard outputs); *out is malloc'ed. */
int vg_filter_pairs(int k, int min_kmers, double min_ident, const int64_t* set_sizes, int64_t n_genomes,
                    const vg_pair_count* pairs, int64_t n_pairs, vg_pair_count** out, int64_t* n_out);

typedef struct {            /* mirrors the prefilter sub-parser, vclust.py:208-262 */
    int    k;               /* -k, 15..30 */
    int    min_kmers;       /* --min-kmers */
    double min_ident;       /* --min-ident */
    int    batch_size;      /* --batch-size: accepted, results do not depend on it */
    double kmers_fraction;  /* --kmers-fraction */
    int    max_seqs;        /* --max-seqs */
    int    num_threads;     /* host threads for ingest */
    int    verbosity;
    int    is_multifasta;   /* args.is_multifasta (vclust.py:689-693) */
} vg_prefilter_params;
int vg_prefilter(const char* const* fasta_paths, int n_paths, const char* out_path,
                 const vg_prefilter_params* p);
/* vg_prefilter for new genomes against a database: vg_genomes_load_db_new + vg_kmer_shared_new + vg_write_fltr.  fltr.txt has the
 * header over all n names and one row per genome; the database rows are empty (`name,`) and a new genome's row holds its partners
 * among the database and the earlier new genomes: the all-vs-all file of the concatenated input with the first n_db rows emptied.
 * (`kmer-db new2all` + distance; no vclust.py call site.) */
int vg_prefilter_new(const char* const* db_paths, int n_db_paths, const char* const* new_paths, int n_new_paths,
                     const char* out_path, const vg_prefilter_params* p);
/* on != 0: the process ends right after its vg_prefilter / vg_align call, so the call leaves the genome set (GBs of host
 * and device memory) to the process exit instead of releasing it piece by piece first (vclust.py's one-shot processes;
 * no reference call site).  Off by default: an embedding process keeps the normal ownership. */
void vg_set_process_ends_after_call(int on);

/* ------------------------------------------------------------------ align ------------- */
typedef struct { int mal, msl, mrd, mqd, reg, aw, am, ar; } vg_lz_params;  /* vclust.py:363-418 */
typedef struct { uint32_t q, r; } vg_task;       /* ordered pair, ids in input order */
typedef struct { uint32_t n_match, aln_len, n_regions; } vg_pair_stat;     /* L5 integers */
typedef struct {            /* one local alignment, 0-based inclusive; r* in fwd|N|rc space */
    uint32_t task; int32_t qstart, qend, rstart, rend; int32_t n_match;
} vg_region;

/* The constants of the LZ restatement that a handful of events of the reference's 12-genome example decide (DESIGN.md
 * section 2, profiles/r04_lz_fit_leave_one_out.md) -- everything else of the parse is held by dozens to thousands of
 * golden regions.  Process-wide; NULL restores the fitted values.  No reference call site: lz-ani has no such options;
 * they exist so that a maintainer with the upstream binaries can re-decide them (tools/compare_with_upstream.py).
 *   weak_seed_ratio  3   R3: a seed shorter than 1/ratio of the literal run it bridges gives one symbol of the anchor
 *                        margin away (0 = never)                                                  [one event]
 *   anchor_margin   -1   R3: a far anchor replaces the seed when longer by MORE than this; -1 = msl - 1 (6 against 7: two pairs)
 *   seed_choice      3   R3: among seeds 3 = longest, then closest to the prediction; 1 = closest, then longest   [three regions]
 * (The fourth thin constant, the oracle's strand separator -- two pairs --, has no counterpart here: the kernels keep one
 * separator symbol and confine every match, extension, window and gap score to its strand by bounds.) */
typedef struct { int weak_seed_ratio, anchor_margin, seed_choice; } vg_lz_fit;
void vg_set_lz_fit(const vg_lz_fit* f);

/* LZ parse of every task on the GPU.  stats: n_tasks entries (caller-owned).
 * regions/n_regions may be NULL; otherwise all kept regions, vg_free(): rows and regions come from ONE parse (round 6); the
 * regions of a task are contiguous and in query order (tasks in the library's reference-grouped order: sort on `task` if
 * the caller's order is needed -- vg_write_ani does). */
int vg_lz_align(vg_genomes* g, const vg_task* tasks, int64_t n_tasks, const vg_lz_params* p,
                vg_pair_stat* stats, vg_region** regions, int64_t* n_regions);

/* Optional head start of vg_lz_align (no reference call site: lz-ani is one process): the indexes of the genomes named
 * by the candidate pairs are planned and the first batch is queued on the device at once, so that they are built while
 * the caller assembles the task list (vg_align_tasks).  vg_lz_align takes them over when its tasks name exactly these
 * references under the same parameters; otherwise they are dropped.  Results never depend on it. */
int vg_lz_prepare(vg_genomes* g, const vg_pair_count* pairs, int64_t n_pairs, const vg_lz_params* p);

/* L1: stable sort by length, descending.  order[rank] = input index. */
int vg_align_order(const vg_genomes* g, int32_t* order /* n */);
/* L2: candidate pairs (input-order ids, a > b) from a Kmer-db filter file with value >= thr,
 * or all pairs when path == NULL */
int vg_read_filter(const vg_genomes* g, const char* path, double thr,
                   vg_pair_count** pairs, int64_t* n_pairs);

/* L7: the canonical ordered-pair list of a candidate set: for ranks a < b the couple
 * (q = b, r = a), (q = a, r = b), couples ascending in (a, b).  ids are input-order ids. */
int vg_align_tasks(const vg_genomes* g, const vg_pair_count* pairs, int64_t n_pairs,
                   vg_task** tasks, int64_t* n_tasks);
/* parity tests: the index vg_lz_align would build for genome `idx` under p (no reference call site).  bucket_end: 4^msl
 * words, the END of each bucket in `entries`; entries: *n_entries words, pos | tag << pos_bits; path: the build that made
 * it, 0..5 the register build of 24, 20, 16, 12, 8, 4 trips, 6 mid, 7 lds, 8 global.  Both arrays: vg_free(). */
int vg_lz_index_dump(vg_genomes* g, int idx, const vg_lz_params* p,
                     uint32_t** bucket_end, uint32_t** entries, int64_t* n_entries,
                     int* pos_bits, int* tag_bits, int* path);
/* HBM budget (bytes) for the per-reference indexes of one vg_lz_align batch (default 24 GiB; without a call a set whose
 * indexes all fit in twice the default is built as one batch) */
void vg_set_index_budget(int64_t bytes);
/* vg_kmer_shared cuts sets that exceed the 32-bit row numbering of one pass (2^32 padded bases)
 * into sub-shards of the k-mer range automatically -- the role of `--batch-size` in the
 * reference (vclust.py:229-239, 1403-1442); n > 0 forces that many sub-shards (tests), 0 = automatic. */
void vg_set_subshards(int n);
/* How one RANGE shard call of vg_kmer_shared (shard / n_shards, sets below 2^32 bases) obtains its kept k-mers:
 * 0 (default) = it scans every base of the set itself; 1 = the sliced scan of the multi-GPU path (rank `shard` scans 1/n_shards
 * of the bases and receives the kept masks and level-1 counts of its k-mer range from the others) with the peers' slices
 * computed by this process: one GPU stands in for the world (tools/strong_scaling_sim.py, tests).  Results are identical.
 * vg_kmer_shared_sharded always exchanges when the sliced scan applies; no reference call site (kmer-db is one process). */
void vg_set_range_scan(int mode);
/* Placement trials: the first dense whole-set pass of vg_kmer_shared in a long-lived process may
 * repeat itself on up to n freshly allocated workspaces and keep the fastest placement (same results; ~0.25 s per
 * placement at 100 k genomes, once).  n <= 1 = none, THE DEFAULT: an embedding application opts in (bench.py does, and
 * says so in its line).  Any failure inside a trial pass is swallowed: the call returns what its first pass computed.
 * No reference call site (kmer-db is one process per call). */
void vg_set_placement_trials(int n);

typedef struct {            /* mirrors the align sub-parser and cmd_lzani, vclust.py:290-421, 1142-1181 */
    vg_lz_params lz;
    double out_tani, out_gani, out_ani, out_qcov, out_rcov;   /* 0 = off */
    const char* filter_path; double filter_threshold;         /* NULL = all-vs-all */
    const char* out_aln_path;                                 /* NULL = none */
    const char* const* out_columns; int n_out_columns;        /* ALIGN_OUTFMT[fmt] */
    int num_threads; int verbosity; int is_multifasta;
} vg_align_params;
/* L6-L8: rows + ids file (+ alignment table when regions != NULL and out_aln_path set).
 * tasks/stats: 2 entries per unordered pair, (q=hi-rank, r=lo-rank) then the reverse. */
int vg_write_ani(const vg_genomes* g, const vg_task* tasks, const vg_pair_stat* stats,
                 int64_t n_tasks, const vg_region* regions, int64_t n_regions,
                 const char* out_path, const vg_align_params* p);
int vg_align(const char* const* fasta_paths, int n_paths, const char* out_path,
             const vg_align_params* p);

/* vg_align for new genomes against a database (no vclust.py call site; lz-ani itself aligns what its filter names).  With
 * p->filter_path it is vg_align on the combined set -- a filter written by vg_prefilter_new names only pairs with a new genome;
 * without one it aligns every pair that contains a new genome.  The ids file lists all n genomes; ani.tsv and the alignment
 * table hold only those pairs.  Indexes are built for the genomes the tasks name and no others, as in vg_align. */
int vg_align_new(const char* const* db_paths, int n_db_paths, const char* const* new_paths, int n_new_paths,
                 const char* out_path, const vg_align_params* p);

/* ------------------------------------------------------------------ one process per GPU - */
/* The reference is single-node / thread-parallel (no distributed layer); these entry points
 * shard the two stages over `world` processes, one GPU each (vg_set_device before the first call).  The only
 * communication is an all-gather of integer records, supplied as a vg_comm:
 *   vg_comm_create       the host application's own exchange (MPI_Allgather, torch.distributed, ...): the callback
 *                        gathers `bytes` bytes from every rank into recv (world * bytes, rank order); on_device != 0
 *                        means send / recv are device pointers of the current HIP device, else host pointers
 *   vg_comm_rccl_create  built-in: RCCL (ncclAllGather over xGMI) on the library's stream; rank 0 obtains the
 *                        128-byte id with vg_rccl_unique_id and hands it to the other ranks by any means
 * A rank that fails -- in its shard, in an allocation, in a merge -- makes every rank return the error: every compute
 * section between two exchanges feeds its status into the next agreement.  VG_DIST_FORCE=1 (tests) runs the exchanges
 * with a world of one. */
typedef struct vg_comm vg_comm;
typedef int (*vg_allgather_fn)(void* ctx, const void* send, void* recv, int64_t bytes, int on_device);
int  vg_comm_create(int rank, int world, vg_allgather_fn allgather, void* ctx, vg_comm** out);
int  vg_rccl_unique_id(void* out /* >= 128 bytes */, int64_t bytes);
int  vg_comm_rccl_create(int rank, int world, const void* unique_id, int64_t id_bytes, vg_comm** out);
void vg_comm_free(vg_comm* c);
/* 1 = built-in RCCL communicator, 0 = callback communicator; the number of ranks RCCL itself reports for the communicator
 * (ncclCommCount; -1 when it is not an RCCL communicator): a scaling record states which exchange it measured */
int  vg_comm_kind(const vg_comm* c);
int  vg_comm_rccl_ranks(const vg_comm* c);
int  vg_comm_rank(const vg_comm* c);
int  vg_comm_world(const vg_comm* c);
/* exchange self-test: every rank sends a pattern of `bytes` bytes and checks what it receives (no GPU needed
 * for a callback communicator over host memory) */
int  vg_comm_selftest(const vg_comm* c, int64_t bytes);
/* vg_kmer_shared over all ranks: rank r counts the k-mers of range r and keeps its partial (a, b, count)
 * list in HBM.  Sets below 2^32 bases (RANGE shards, two partition levels): every rank scans 1/world of the BASES and an
 * all-to-all (RCCL: grouped ncclSend / ncclRecv, one xGMI link per peer) hands each rank the kept-k-mer masks (one bit per
 * base) and level-1 counts of its own range -- no rank computes a k-mer it does not keep or forward.  Exchanged after that: the set sizes, the KEYS of the pairs a rank holds >= ceil(min_shared / world) of (a pair
 * that reaches min_shared in total has that many on some rank), and every rank's count for each pair of the union of
 * those keys; the counts are summed and the threshold is applied to the SUM.  Every rank receives the global result,
 * sorted by (a, b); device-to-device all-gathers only. */
int vg_kmer_shared_sharded(vg_genomes* g, int k, double fraction, uint32_t min_shared, const vg_comm* c,
                           int64_t* set_sizes, vg_pair_count** pairs, int64_t* n_pairs);
/* owner rank of every task: references cut into `world` contiguous id ranges with about equal task counts */
int vg_align_owner(const vg_task* tasks, int64_t n_tasks, int n_genomes, int world, int32_t* owner /* n_tasks */);
/* vg_lz_align over all ranks (reference-range partition): every rank receives all rows (and regions) */
int vg_lz_align_sharded(vg_genomes* g, const vg_task* tasks, int64_t n_tasks, const vg_lz_params* p, const vg_comm* c,
                        vg_pair_stat* stats, vg_region** regions, int64_t* n_regions);
/* rank `rank`'s share of the align tasks of the candidate pairs under the reference-range partition (a pure function of
 * the pairs; tasks in pair order, (q = b, r = a) before (q = a, r = b)); *tasks released with vg_free() */
int vg_align_pairs_share(const vg_genomes* g, const vg_pair_count* pairs, int64_t n_pairs, int world, int rank,
                         vg_task** tasks, int64_t* n_tasks);
/* (every rank passes the SAME pairs in the SAME order -- vg_kmer_shared_sharded returns them sorted; a checksum of the list
 * is compared across the ranks and a difference is an error on all of them) */
/* vg_align_tasks + vg_lz_align_sharded from the candidate pairs in one call: a rank derives its own tasks from the pairs
 * and starts its kernels at once, the canonical task list of the whole set is assembled beside them and only places the
 * gathered rows.  *tasks (canonical order, as vg_align_tasks) and *stats (one row per task) are released with vg_free(). */
int vg_lz_align_pairs_sharded(vg_genomes* g, const vg_pair_count* pairs, int64_t n_pairs, const vg_lz_params* p, const vg_comm* c,
                              vg_task** tasks, int64_t* n_tasks, vg_pair_stat** stats);
/* the two whole stages (vg_prefilter / vg_align) on `world` GPUs: every rank ingests the FASTA, rank 0 writes */
int vg_prefilter_sharded(const char* const* fasta_paths, int n_paths, const char* out_path,
                         const vg_prefilter_params* p, const vg_comm* c);
int vg_align_sharded(const char* const* fasta_paths, int n_paths, const char* out_path,
                     const vg_align_params* p, const vg_comm* c);

/* ------------------------------------------------------------------ cluster ----------- */
/* The third stage: ani.tsv + ids file -> clusters.tsv, in place of Clusty (cmd_clusty, vclust.py:1184-1278, run at
 * vclust.py:1539-1557) for the four algorithms with a deterministic definition; DESIGN.md section 9 is the contract.
 * Objects are the rows of the ids file (index = row number from 0, i.e. the align stage's length order).  A row of ani.tsv
 * passes when every minimum > 0 holds (column >= value), num_alns <= max_num_alns when that is > 0, and qidx != ridx; it
 * links {qidx, ridx} with the metric value as weight (the maximum over duplicate and reverse rows). */
enum { VG_CLUSTER_SINGLE = 0, VG_CLUSTER_CDHIT = 1, VG_CLUSTER_UCLUST = 2, VG_CLUSTER_SET_COVER = 3, VG_CLUSTER_COMPLETE = 4, VG_CLUSTER_AVERAGE = 5,
       VG_CLUSTER_MCL = 6 /* Markov clustering: its own calls below; vg_cluster and vg_cluster_graph refuse it */ };
typedef struct {            /* mirrors the cluster sub-parser, vclust.py:423 ff. */
    int algorithm;                                            /* VG_CLUSTER_* */
    const char* metric;                                       /* "tani" | "gani" | "ani": the edge weight */
    double min_tani, min_gani, min_ani, min_qcov, min_rcov, min_len_ratio;     /* 0 = off */
    int max_num_alns;                                         /* 0 = off */
    int representatives;                                      /* second column: the representative's id, not a number */
    int num_threads; int verbosity;
} vg_cluster_params;
typedef struct {
    int64_t rounds;             /* parallel rounds launched (single: hooking rounds; complete, average: merge rounds) */
    int64_t sweep_objects;      /* objects decided by the one-workgroup tail sweep */
    int64_t n_edges;            /* undirected edges after dropping self rows and merging duplicates */
} vg_cluster_stats;
/* The whole stage, file to file: columns are found by header name (any --outfmt); a missing column, an index outside the
 * ids file or a malformed number is VG_EINVAL naming the file and line, reported before any device use.  Output: header
 * `object<TAB>cluster`, one line per object in ids-file order; clusters of >= 2 members are numbered 0, 1, ... by their
 * earliest member, then singletons in ids-file order; with `representatives` the second column is the id of the cluster's
 * earliest member.  VG_CLUSTER_AVERAGE is the average-linkage hierarchy below, run down to the metric's minimum (its floor) with
 * every merge joined; a weight outside [0, 1] is VG_EINVAL for it. */
int vg_cluster(const char* ani_path, const char* ids_path, const char* out_path, const vg_cluster_params* p);
/* The array-level stage: rows (q[i], r[i], w[i]) over n_objects objects, read as above (self rows dropped, duplicates
 * merged to the maximum weight; NaN weights and indices >= n_objects are VG_EINVAL, n_objects >= 2^31 VG_EOVERFLOW).
 * label[n_objects]: the output file's numbering; representative[n_objects]: the index of the cluster's earliest member.
 * stats may be NULL.  VG_CLUSTER_COMPLETE (here and in vg_cluster) is the cut of the complete-linkage hierarchy below at the
 * floor, i.e. after every merge: each cluster is a clique of passing rows; sweep_objects is 0.  VG_CLUSTER_AVERAGE needs a
 * floor, which this call does not take: it is VG_EINVAL here (use the average-linkage calls below). */
int vg_cluster_graph(int64_t n_objects, const uint32_t* q, const uint32_t* r, const double* w, int64_t n_edges,
                     int algorithm, int32_t* label, int32_t* representative, vg_cluster_stats* stats);

/* Update of a prior clustering (this repository's definition; DESIGN.md section 9, "Update of a prior clustering"): new objects
 * are added to clusters that are taken as given.  Objects with a prior cluster are *prior*, the others *new*; the visit order is
 * the prior objects in index order, then the new ones in index order.  Rows are read as above, and a row between two prior
 * objects is ignored.  VG_CLUSTER_CDHIT / VG_CLUSTER_UCLUST: every prior object keeps its cluster and every prior cluster its
 * representative; the new objects are visited in visit order and join the earliest (cd-hit) or heaviest (uclust; ties: earliest)
 * representative, prior or new, they have an edge to, else found a cluster.  VG_CLUSTER_SINGLE: the connected components of the
 * prior partition plus the kept edges (prior clusters may merge); the representative is the earliest member by index. */
typedef struct {
    int64_t rounds, sweep_objects, n_edges;     /* as vg_cluster_stats; n_edges counts the kept edges only */
    int64_t n_prior, n_new;                     /* objects with / without a prior cluster */
    int64_t joined_prior, joined_new, founded;  /* new objects by outcome: joined a prior representative, joined a new one, founded a
                                                 * cluster (single: joined_new = 0, founded = new objects in components without a prior object) */
    int64_t prior_merged;                       /* single: prior clusters minus components that contain a prior object; 0 otherwise */
} vg_cluster_update_stats;
/* The array-level update.  prior_rep[n_objects]: -1 for a new object, else the index of the representative of the object's prior
 * cluster (prior_rep[prior_rep[i]] == prior_rep[i]; it need not be the cluster's earliest member).  A value outside [-1, n_objects)
 * or a representative that is not its own representative is VG_EINVAL, as is an algorithm other than the three above; every
 * argument check runs on the host before any device use.  label[n_objects]: the numbering of vg_cluster_graph applied to the
 * final partition (by earliest member); representative[n_objects]: the frozen or founding representative (cd-hit, uclust) or the
 * earliest member (single).  stats may be NULL.  No device is VG_ENODEV, n_objects >= 2^31 VG_EOVERFLOW. */
int vg_cluster_update_graph(int64_t n_objects, const uint32_t* q, const uint32_t* r, const double* w, int64_t n_rows,
                            int algorithm, const int32_t* prior_rep, int32_t* label, int32_t* representative,
                            vg_cluster_update_stats* stats);
/* File to file, with the host parse and the error messages of vg_cluster.  prior_path: a clusters.tsv of this library (header
 * `object<TAB>cluster`, one line per prior object), matched to the ids file by name.  Column 2 is a cluster number, and the
 * representative of a prior cluster is then its earliest member in the ids file; with prior_is_repr it is the representative's id
 * (as p->representatives writes it), which must be an object of the prior file and its own representative.  A name that is not
 * in the ids file, a name listed twice, a malformed line or such a representative is VG_EINVAL naming the file and line, reported
 * before any device use.  out_path: clusters.tsv of vg_cluster for the final partition; with p->representatives the second
 * column is the representative above (a frozen one even where a new member comes earlier in the ids file). */
int vg_cluster_update(const char* ani_path, const char* ids_path, const char* prior_path, int prior_is_repr,
                      const char* out_path, const vg_cluster_params* p, vg_cluster_update_stats* stats);

/* Single-linkage merge table and multi-level cuts (this repository's; DESIGN.md section 9, "Merge table").  The graph is the
 * one above.  Edge {a, b} (a < b) of weight w has the key (-w, a, b), weights compared as doubles with -0.0 = +0.0: a strict
 * total order.  Kruskal over the edges in key order; an edge whose ends lie in different clusters is a merge, and there are
 * n_objects - (number of components) of them: the maximum spanning forest, computed on the device.  Objects are nodes
 * 0 .. n_objects - 1 and merge k (from 0) creates node n_objects + k.  The cut at level t joins the merges with w >= t; its
 * labels and representatives follow the rule of vg_cluster_graph, and it equals `single` on the rows with w >= t. */
typedef struct {
    int64_t rounds;             /* single: Boruvka rounds launched (the last one finds no leaving edge); complete, average: merge rounds */
    int64_t n_edges;            /* undirected edges after dropping self rows and merging duplicates */
    int64_t n_merges;           /* single: forest edges = n_objects - components; complete, average: n_objects - clusters at the floor */
} vg_linkage_stats;
/* The merge table of the rows (validated as vg_cluster_graph validates them, before any device use).  Every output array is the
 * caller's and has n_objects - 1 entries (they may be NULL when n_objects <= 1); *n_merges of them are written, in merge order:
 * the edge (object_a < object_b, weight), the two nodes merged (node_a < node_b) and the members of the new node.  stats may be
 * NULL.  No device is VG_ENODEV, n_objects >= 2^31 VG_EOVERFLOW. */
int vg_cluster_linkage_graph(int64_t n_objects, const uint32_t* q, const uint32_t* r, const double* w, int64_t n_rows,
                             int32_t* object_a, int32_t* object_b, double* weight, int64_t* node_a, int64_t* node_b,
                             int64_t* size, int64_t* n_merges, vg_linkage_stats* stats);
/* The cuts of ONE forest at levels[0 .. n_levels): label and representative hold n_levels rows of n_objects entries each, in the
 * order of the levels (any order, repeats allowed; a NaN level is VG_EINVAL). */
int vg_cluster_levels_graph(int64_t n_objects, const uint32_t* q, const uint32_t* r, const double* w, int64_t n_rows,
                            const double* levels, int n_levels, int32_t* label, int32_t* representative, vg_linkage_stats* stats);
/* Complete-linkage merge table and cuts (this repository's definition; DESIGN.md section 9, "Merge table: complete linkage").
 * Same graph, same edge key (-w, a, b); a pair of objects without an edge has the key +infinity.  K(A, B) of two clusters is the
 * LARGEST key over all pairs a in A, b in B (the worst pair; +infinity when any pair has no edge).  From singletons, the two
 * clusters of smallest finite K merge, until no finite K is left; the merge record is that worst edge (object_a < object_b,
 * weight).  Every cluster is a clique of passing rows, records come in increasing key order (weights never rise), and the table,
 * node numbering, cuts, labels and representatives are exactly those of the single-linkage calls.  The cut at level t equals
 * the run on the rows with w >= t after every merge.  On the device the merges of mutually nearest clusters happen in parallel
 * rounds (the linkage is reducible, so these are the merges of the sequential rule); stats->rounds counts the merge rounds
 * launched (the last one finds no merge).  Arguments, outputs and errors as vg_cluster_linkage_graph / vg_cluster_levels_graph. */
int vg_cluster_complete_linkage_graph(int64_t n_objects, const uint32_t* q, const uint32_t* r, const double* w, int64_t n_rows,
                                      int32_t* object_a, int32_t* object_b, double* weight, int64_t* node_a, int64_t* node_b,
                                      int64_t* size, int64_t* n_merges, vg_linkage_stats* stats);
int vg_cluster_complete_levels_graph(int64_t n_objects, const uint32_t* q, const uint32_t* r, const double* w, int64_t n_rows,
                                     const double* levels, int n_levels, int32_t* label, int32_t* representative, vg_linkage_stats* stats);
/* Average-linkage (UPGMA) merge table and cuts (this repository's definition; DESIGN.md section 9, "Merge table: average linkage").
 * Same graph; every weight must be finite and in [0, 1] (else VG_EINVAL, before any device use), and so must `floor`.  A weight w
 * is the integer u = llrint(ldexp(w, 32)), and everything else is integer arithmetic on u: S(A, B) is the sum of u over the edges
 * between two clusters, P(A, B) = |A| * |B|, sim(A, B) = S / (P * 2^32) -- a pair of objects without an edge adds 0 to S and 1 to P.
 * A pair of clusters with at least one edge between them is a candidate with the key (-sim, c, d), c < d the cluster ids (minimum
 * members), sim compared exactly (S1 * P2 against S2 * P1 in 128 bits).  From singletons, the candidate of smallest key merges,
 * until none is left or the smallest key has sim < floor (S < F * P, F = llrint(ldexp(floor, 32))).  Record k: object_a < object_b
 * are the two cluster ids merged, sum = S, pairs = P, similarity = the double nearest to S / (P * 2^32) (ties to even); similarity
 * never rises down the table, and node numbering, labels and representatives are those of the calls above.  The cut at level t
 * joins the merges with S >= T * P, T = llrint(ldexp(t, 32)); a level below the floor is VG_EINVAL.  Unlike the other two
 * hierarchies, the cut at t is NOT the floor cut of a run with floor t: the rows between the floor and t still count in the
 * averages.  2^32 or more edges are VG_EOVERFLOW.  stats->rounds counts the merge rounds launched (the last one finds no merge).
 * sum and pairs have n_objects - 1 entries like the other outputs. */
int vg_cluster_average_linkage_graph(int64_t n_objects, const uint32_t* q, const uint32_t* r, const double* w, int64_t n_rows,
                                     double floor, int32_t* object_a, int32_t* object_b, double* similarity, uint64_t* sum,
                                     uint64_t* pairs, int64_t* node_a, int64_t* node_b, int64_t* size, int64_t* n_merges,
                                     vg_linkage_stats* stats);
int vg_cluster_average_levels_graph(int64_t n_objects, const uint32_t* q, const uint32_t* r, const double* w, int64_t n_rows,
                                    double floor, const double* levels, int n_levels, int32_t* label, int32_t* representative,
                                    vg_linkage_stats* stats);
/* Test entries of that arithmetic.  The double nearest to sum / (pairs * 2^32), ties to even (host code; pairs == 0 gives NaN). */
double vg_cluster_average_similarity(uint64_t sum, uint64_t pairs);
/* out[i], i in 0 .. n - 2, is -1, 0 or 1 as entry i has the smaller, the same or the larger key than entry i + 1, where entry i is
 * the candidate of similarity sum[i] / (size_c[i] * size_d[i]) between the clusters c[i] and d[i]: the comparator the kernels and the
 * host share, run on the host or (on_device != 0; VG_ENODEV without one) in one kernel launch. */
int vg_cluster_average_order_selftest(const uint64_t* sum, const uint32_t* size_c, const uint32_t* size_d, const uint32_t* c,
                                      const uint32_t* d, int64_t n, int on_device, int8_t* out);
/* File to file, with the host parse and the error messages of vg_cluster; p->algorithm must be VG_CLUSTER_SINGLE,
 * VG_CLUSTER_COMPLETE or VG_CLUSTER_AVERAGE (else VG_EINVAL) and selects the hierarchy; the floor of VG_CLUSTER_AVERAGE is the
 * metric's minimum.  out_path: clusters.tsv of vg_cluster (the cut at the metric's floor) plus one column per level, headed
 * `<metric>_<%g of the level>`, labels or -- with p->representatives -- representative ids; a level below the metric's minimum
 * is VG_EINVAL.  linkage_path (may be NULL): header `node_a node_b similarity size object_a object_b` (tab-separated), one line
 * per merge, similarity printed with %.6g. */
int vg_cluster_linkage(const char* ani_path, const char* ids_path, const char* out_path, const vg_cluster_params* p,
                       const char* linkage_path, const double* levels, int n_levels);

/* Cluster report: cohesion and separation of a given clustering (this repository's definition; DESIGN.md section 9, "Cluster
 * report").  The graph is the one above, every weight finite and in [0, 1] (else VG_EINVAL, before any device use) and taken as the
 * integer u = llrint(ldexp(w, 32)) of average linkage; every figure is integer arithmetic on u.  label[i] in [0, n_clusters) is the
 * cluster of object i -- any partition, computed by this library or not.  One record per label; a label without members has size 0,
 * rep and nearest -1 and every other field 0. */
typedef struct {
    int64_t size;               /* members */
    int64_t rep;                /* the earliest member (minimum index) */
    uint64_t pairs;             /* size * (size - 1) / 2 */
    uint64_t linked;            /* edges with both ends in the cluster */
    uint64_t sum, min;          /* sum and minimum of u over those edges (min = 0 when linked == 0) */
    uint64_t external;          /* edges with exactly one end in the cluster */
    int64_t nearest;            /* the other label with the largest u on an edge between the two (ties: the smallest label); -1 when external == 0 */
    uint64_t nearest_max;       /* that largest u */
    uint64_t nearest_sum;       /* sum of u over all edges between the cluster and `nearest` */
    int64_t misfits;            /* members with other_max > own_max (below) */
} vg_cluster_stat;
/* The array-level report: rows as passed to vg_cluster_graph (already-passing rows), out[n_clusters].  Per object, each array of
 * n_objects entries or NULL: own_max[i] = the largest u to a member of its own cluster (0 without one), other_max[i] = the largest u
 * to an object of another cluster (0 without one) and other[i] = that object's label (ties: the smallest label; -1 without one).
 * n_objects == 0 and n_rows == 0 are valid.  A label outside [0, n_clusters) is VG_EINVAL (checked on the host before any device
 * use), n_objects or n_clusters >= 2^31 and 2^32 or more undirected edges VG_EOVERFLOW, no device VG_ENODEV (no host fallback). */
int vg_cluster_stats_graph(int64_t n_objects, const uint32_t* q, const uint32_t* r, const double* w, int64_t n_rows,
                           const int32_t* label, int64_t n_clusters, vg_cluster_stat* out, uint64_t* own_max, uint64_t* other_max,
                           int32_t* other);
/* File to file, made after clusters.tsv is written: the rows of ani.tsv that pass p's filters (the parse and the error messages
 * of vg_cluster; p->algorithm and p->representatives are not read), then clusters_path -- header `object` and one or more label
 * columns, objects matched to the ids file by name, every id exactly once; a label is a non-negative integer or, with
 * clusters_is_repr, the id of a member of that cluster.  Anything else is VG_EINVAL naming the file and line, before any device
 * use.  out_path: tab-separated, header `column cluster size representative pairs linked min_<metric> mean_linked mean_all external
 * nearest nearest_<metric> nearest_mean misfits`; one block per label column in file order (`column` = its header), one line per
 * cluster ordered by its earliest member; `cluster` and `nearest` are the label texts of clusters_path; the quotients
 * (sum / (linked * 2^32), sum / (pairs * 2^32), nearest_sum / (size * size[nearest] * 2^32), min / 2^32, nearest_max / 2^32) are the
 * doubles nearest the exact values, printed %.6g, and `-` where there is no denominator, no linked edge or no nearest cluster. */
int vg_cluster_stats_file(const char* ani_path, const char* ids_path, const char* clusters_path, int clusters_is_repr,
                          const vg_cluster_params* p, const char* out_path);

/* Markov clustering (this repository's definition; DESIGN.md section 9, "Markov clustering"; tests/mcl_restatement.py is the
 * sequential restatement).  The graph is the one above, every weight in [0, 1] (else VG_EINVAL).  The flow matrix is held in
 * integers: an entry is a uint32 in units of 2^-30 (ONE = 2^30), row i the flow out of object i.  Start: the quantised weights
 * llrint(w * 2^32), a loop as heavy as the row's heaviest edge (ONE without edges), the row normalised (p = floor(x * ONE / sum),
 * zeros dropped).  One iteration, per row: expansion (the row times the matrix, exact 64-bit sums, >> 30), inflation by
 * inflation = a / 2 (an exact integer square root when a is odd, then a >> 1 multiplications, each >> 30; zeros dropped; nothing left:
 * the row is the loop alone), normalisation, pruning (entries >= floor(prune * ONE), else the largest; at most the max_row largest by
 * (value descending, column ascending)), normalisation again; the row's chaos is max p - (sum p^2 >> 30).  The run stops after the
 * first iteration whose largest chaos is <= floor(chaos_eps * ONE) (converged = 1) or after max_iterations (converged = 0: there
 * is a result all the same).  Clusters: the connected components of {i, j : p_ij > 0, i != j} of the last matrix, labelled as
 * VG_CLUSTER_SINGLE labels them.  Every sum is an integer sum: the result does not depend on the order of anything. */
typedef struct {
    double inflation;           /* a multiple of 0.5 in [1.5, 6] (pow() is not correctly rounded on the device; halves are exact) */
    double prune;               /* [0, 0.1] */
    double chaos_eps;           /* [0, 1) */
    int max_row;                /* [2, 4096] */
    int max_iterations;         /* [1, 1000] */
} vg_mcl_params;
typedef struct {
    int64_t iterations, converged;
    int64_t n_edges;            /* undirected edges after dropping self rows and merging duplicates */
    int64_t nnz, max_row_seen;  /* entries and widest row of the last matrix */
    int64_t lds_rows, spill_rows;   /* rows expanded in an LDS table / through the sorted spill records, over all iterations */
    uint64_t chaos;             /* of the last iteration, in units of 2^-30 */
} vg_mcl_stats;
/* Rows as for vg_cluster_graph.  A parameter outside its range is VG_EINVAL naming it; every argument check runs on the host before
 * any device use; n_objects == 0 is VG_OK without a device, n_objects >= 2^31 VG_EOVERFLOW, no device VG_ENODEV.  m_off, m_col and
 * m_val may all be NULL; otherwise they receive the last matrix as CSR (m_off[n_objects + 1], columns ascending per row), each to be
 * released with vg_free: with max_iterations = t that is the iterate after t steps.  stats may be NULL. */
int vg_cluster_mcl_graph(int64_t n_objects, const uint32_t* q, const uint32_t* r, const double* w, int64_t n_rows,
                         const vg_mcl_params* params, int32_t* label, int32_t* representative, int64_t** m_off, int32_t** m_col,
                         uint32_t** m_val, vg_mcl_stats* stats);
/* File to file, with the host parse, the output and the error messages of vg_cluster; p->algorithm must be VG_CLUSTER_MCL. */
int vg_cluster_mcl(const char* ani_path, const char* ids_path, const char* out_path, const vg_cluster_params* p,
                   const vg_mcl_params* params, vg_mcl_stats* stats);
/* Developer knob: the slots of the LDS table a row may use (a power of two in 16..4096; 0 = the default, 4096).  A row whose
 * candidate bound exceeds it and whose distinct columns fill more than 3/4 of it takes the spill path, so a small value sends
 * tiny graphs there. */
void vg_cluster_mcl_set_table_slots(int slots);

/* ------------------------------------------------------------------ coverage ---------- */
/* Coverage map (this repository's definition; DESIGN.md section 14 is the contract, tests/cover_restatement.py its sequential
 * statement).  n objects with lengths len[i]; optionally a group label[i] in [0, n_groups) per object (NULL: one group).  A row
 * (q, r, qstart, qend) says that the positions qstart..qend (0-based, inclusive) of object q are aligned to partner r; only the
 * query side counts and a row with q == r is ignored.  C(i, r) is the union of the rows (i, r, ..); depth_in(x) / depth_out(x) of
 * object i count the partners r of i's group / of another group with x in C(i, r).  The segments of an object with len > 0 are the
 * maximal runs on which (depth_in, depth_out) is constant: disjoint, covering 0..len-1, ordered by (object, start); an object
 * without rows has the one segment (0, len-1, 0, 0).  The result depends on the set of rows only. */
typedef struct {
    int64_t len;
    int64_t partners_in, partners_out;              /* distinct partners with a row, of the object's group / of another */
    int64_t covered, covered_in, covered_out;       /* positions with depth_in + depth_out >= 1, depth_in >= 1, depth_out >= 1 */
    int64_t core;               /* positions with depth_in == (members of the group) - 1; 0 for a group of one */
    int64_t sum_in, sum_out;    /* the depths summed over the positions = |C(i, r)| summed over the partners */
    int64_t max_depth;          /* the largest depth_in + depth_out */
    int64_t segments;           /* the object's segments */
} vg_cover_stat;
typedef struct { int32_t object, start, end, depth_in, depth_out; } vg_cover_segment;   /* 0-based inclusive */
typedef struct {
    int64_t rows_kept;          /* rows with q != r */
    int64_t intervals;          /* maximal intervals of all C(i, r) (rows that overlap or touch are one) */
    int64_t breakpoints;        /* distinct (object, position) at which an interval starts or has just ended */
    int64_t segments;
} vg_cover_run_stats;
/* out[n_objects].  segments / n_segments: both NULL (no profile) or both given; *segments is released with vg_free.  Checked on
 * the host before any device use, VG_EINVAL naming the row or object: an index >= n_objects, qstart < 0, qstart > qend,
 * qend >= len[q], a negative length or one >= 2^31, a label outside [0, n_groups), only one of segments / n_segments.
 * n_objects >= 2^31 or n_rows >= 2^32 is VG_EOVERFLOW; n_objects == 0 is VG_OK without a device; no device VG_ENODEV (no host
 * fallback).  st may be NULL. */
int vg_cover_rows(int64_t n_objects, const int64_t* len, const int32_t* label, int64_t n_groups,
                  const uint32_t* q, const uint32_t* r, const int32_t* qstart, const int32_t* qend, int64_t n_rows,
                  vg_cover_stat* out, vg_cover_segment** segments, int64_t* n_segments, vg_cover_run_stats* st);
/* File to file.  ids_path: the ids file of vg_align (columns `id` first and `seq_len`, found by header name).  aln_path: the table
 * vg_align writes with out_aln_path; the columns query, reference, qstart, qend are found by header name and hold 1-based inclusive
 * positions; names are matched to the ids file.  clusters_path (may be NULL: one group): read as by vg_cluster_stats_file; column
 * (NULL: the first) names the label column that gives the groups.  An unknown name, a missing column, a malformed number, a range
 * outside 1..seq_len or an unknown label column is VG_EINVAL `<file>:<line>: ...`, before any device use.  out_path: tab-separated,
 * one line per object in ids-file order, header `id len group group_size partners_in partners_out covered covered_in covered_out
 * core max_depth mean_depth covered_frac core_frac`; group is the label text of clusters_path (`-` without one); the quotients
 * (sum_in + sum_out) / len, covered / len and core / len are printed %.6g, `-` when len == 0, and core_frac also when
 * group_size < 2.  segments_path (may be NULL): header `id start end depth_in depth_out`, positions 1-based inclusive, in segment
 * order.  The bytes do not depend on num_threads.  verbosity >= 1: one summary line on stderr. */
int vg_cover_file(const char* aln_path, const char* ids_path, const char* clusters_path, int clusters_is_repr,
                  const char* column, const char* out_path, const char* segments_path, int num_threads, int verbosity);

/* ------------------------------------------------------------------ painting ---------- */
/* Mosaic painting (this repository's definition; DESIGN.md section 15 is the contract, tests/paint_restatement.py its sequential
 * statement).  Objects, lengths and groups as in the coverage map.  A row (q, r, qstart, qend, n_match) says that the positions
 * qstart..qend (0-based, inclusive) of object q are aligned to partner r with n_match matching positions, 0 <= n_match <= span =
 * qend - qstart + 1; only the query side counts and a row with q == r is ignored.  A row outranks another row of the same object by
 * larger I = floor(n_match * 2^32 / span), then larger span, then smaller r, then smaller qstart (rows equal on all four are the same
 * row).  The winner at a position is the best-ranked row that covers it; a position no row covers is unpainted.  The segments of an
 * object with len > 0 are the maximal runs of one winning row, or of no winner: disjoint, covering 0..len-1, ordered by (object,
 * start).  The result depends on the set of rows only. */
typedef struct {
    int64_t len;
    int64_t painted;                    /* positions with a winner */
    int64_t painted_in, painted_out;    /* ... whose partner is of the object's group / of another group */
    int64_t donors;                     /* distinct winning partners */
    int64_t top_partner, top_painted;   /* the donor with the most positions (ties: the smallest index; -1 without one), and how many */
    int64_t switches;                   /* pairs of neighbouring segments, both painted, with different partners */
    int64_t segments;
} vg_paint_stat;
/* 0-based inclusive; an unpainted segment has partner = row_qstart = row_qend = -1 and n_match = 0 */
typedef struct { int32_t object, start, end, partner, row_qstart, row_qend, n_match; } vg_paint_segment;
typedef struct { int32_t object, partner; int64_t painted, segments; } vg_paint_donor;   /* by (object, partner) */
typedef struct {
    int64_t rows_kept;          /* rows with q != r */
    int64_t breakpoints;        /* distinct (object, position) over qstart and qend + 1 of the kept rows, and 0 and len of every object with len > 0 */
    int64_t segments;
    int64_t donor_records;
    int64_t levels;             /* levels of the maximum structure: floor(log2(the longest row in elementary segments)) + 1; 0 without rows */
} vg_paint_run_stats;
/* out[n_objects].  segments / n_segments and donors / n_donors: each pair both NULL or both given; *segments and *donors are
 * released with vg_free.  Checks, limits and codes are those of vg_cover_rows, on the host before any device use, and also
 * VG_EINVAL for n_match < 0 or n_match > span.  n_objects == 0 is VG_OK without a device; no device VG_ENODEV (no host fallback).
 * st may be NULL. */
int vg_paint_rows(int64_t n_objects, const int64_t* len, const int32_t* label, int64_t n_groups,
                  const uint32_t* q, const uint32_t* r, const int32_t* qstart, const int32_t* qend, const int32_t* n_match, int64_t n_rows,
                  vg_paint_stat* out, vg_paint_segment** segments, int64_t* n_segments, vg_paint_donor** donors, int64_t* n_donors,
                  vg_paint_run_stats* st);
/* File to file.  The files are read as by vg_cover_file; the table's columns alnlen and nt_match are taken as well, by header name,
 * and `<file>:<line>: ...` VG_EINVAL also when alnlen != qend - qstart + 1, nt_match > alnlen, or (with a column nt_mismatch)
 * nt_match + nt_mismatch != alnlen.  out_path: one line per object in ids-file order, header `id len group painted painted_in
 * painted_out donors top_partner top_painted switches segments painted_frac top_frac`; top_partner is the partner's id (`-` without
 * one); painted / len and top_painted / len are printed %.6g, `-` when len == 0.  segments_path (may be NULL): header `id start end
 * partner pident row_qstart row_qend`, positions 1-based inclusive, pident = 100 * n_match / span of the winning row in the digits
 * of vg_align's alignment table; the last four are `-` on an unpainted segment.  donors_path (may be NULL): header `id partner
 * painted segments painted_frac`.  The bytes do not depend on num_threads.  verbosity >= 1: one summary line on stderr. */
int vg_paint_file(const char* aln_path, const char* ids_path, const char* clusters_path, int clusters_is_repr, const char* column,
                  const char* out_path, const char* segments_path, const char* donors_path, int num_threads, int verbosity);

/* ------------------------------------------------------------------ dereplicate ------- */
/* Greedy incremental clustering against representatives only (this repository's command; no reference call site; DESIGN.md
 * section 13 is the contract).  Objects are the genomes in align order (vg_align_order; rank = object index, as in ani.ids.tsv).
 * The result is the one of vg_kmer_shared + vg_filter_pairs -> vg_lz_align of every kept pair -> vg_cluster_graph(VG_CLUSTER_CDHIT) on
 * the rows that pass the cluster filters AS ani.tsv PRINTS THEM, but a genome is only ever compared with the representatives found
 * so far and with the batch-mates that joined none of them: per batch of `batch_genomes` consecutive ranks, the working set
 * [representatives | batch] (the batch appended by vg_genomes_extend, dropped again by vg_genomes_truncate, its founders appended for
 * good), vg_kmer_shared_new with the representatives as the database, the pairs (batch
 * genome, representative) aligned first, then the pairs among the batch genomes still without a representative, and
 * vg_cluster_update_graph(VG_CLUSTER_CDHIT) with the representatives as the prior clustering.  The representatives stay in HBM. */
typedef struct {
    int    k;                   /* -k, 15..30 */
    double kmers_fraction;      /* --kmers-fraction, (0, 1] */
    int    min_kmers;           /* --min-kmers */
    double min_ident;           /* --min-ident */
    vg_lz_params lz;
    vg_cluster_params cluster;  /* metric and filters as for vg_cluster; algorithm must be VG_CLUSTER_CDHIT and the metric's minimum > 0 */
    int    batch_genomes;       /* genomes per batch, >= 1; results never depend on it */
} vg_derep_params;
typedef struct {                /* pair counts are unordered pairs */
    int64_t batches;
    int64_t representatives;
    int64_t pairs_candidate;    /* pairs kept by the prefilter, over all batches */
    int64_t pairs_aligned;      /* of those, aligned (both directions) */
    int64_t pairs_skipped;      /* of those, never aligned: a batch genome that joined an earlier representative against its batch-mates */
    int64_t joined_prior;       /* genomes that joined a representative of an earlier batch */
    int64_t joined_new;         /* genomes that joined a representative of their own batch */
    int64_t founded;            /* = representatives */
} vg_derep_stats;
/* The array-level call.  label[n], representative[n]: indexed by object (rank), exactly what vg_cluster_graph(VG_CLUSTER_CDHIT) returns
 * for the passing rows of the whole pair list.  tasks / stats_rows / n_tasks (all three or none; vg_free): every aligned ordered pair
 * in input-order ids with its integers, couples in the order of vg_align_tasks, ready for vg_write_ani.  st may be NULL.  Refused with
 * VG_EINVAL before any device use: batch_genomes < 1, an algorithm other than VG_CLUSTER_CDHIT, an unknown metric, a metric minimum
 * of 0, k outside 15..30, kmers_fraction outside (0, 1].  The representatives the batches found are compared with those of the final
 * vg_cluster_graph over all rows; a difference is an internal error (VG_EHIP) naming the object. */
int vg_dereplicate_set(vg_genomes* g, const vg_derep_params* p, int32_t* label, int32_t* representative, vg_task** tasks,
                       vg_pair_stat** stats_rows, int64_t* n_tasks, vg_derep_stats* st);
typedef struct {
    vg_derep_params derep;
    int representatives;                                      /* clusters.tsv: second column = the representative's id */
    const char* out_table_path;                               /* NULL = none; else ani.tsv of the computed rows + its .ids.tsv (all n genomes) */
    const char* const* out_columns; int n_out_columns;        /* columns of that table (ALIGN_OUTFMT[fmt]) */
    const char* out_repr_fasta_path;                          /* NULL = none; one multi-FASTA input only: the representatives' records, verbatim, input order */
    int num_threads; int verbosity; int is_multifasta;
    vg_derep_stats* stats;                                    /* NULL, or where the counts go */
} vg_derep_file_params;
/* File to file: FASTA in, clusters.tsv (the file vg_cluster writes) out.  verbosity >= 1: one summary line on stderr,
 * `Dereplicate: <n> genomes, <r> representatives, <b> batches, <p> pairs aligned (<c> candidates skipped)`. */
int vg_dereplicate(const char* const* fasta_paths, int n_paths, const char* out_path, const vg_derep_file_params* p);

/* New genomes added to an earlier run ("Update"): the clusters and representatives of a prior clustering are
 * kept as they are, and every other object is dereplicated on top of them.  The result is vg_cluster_update_graph(VG_CLUSTER_CDHIT)
 * over the whole edge graph of vg_dereplicate_set with that prior: new objects are visited in index order and join the earliest
 * representative in visit order (the prior representatives in index order, then the founders), else found a cluster.  Only the prior
 * REPRESENTATIVES are ever gathered, indexed or aligned: a row to a prior member joins nothing.  vg_dereplicate_set is this call
 * with no prior object.  In vg_derep_stats, `representatives` then counts the prior ones too, `founded` the new ones only, and
 * `joined_prior` the new genomes that joined a representative older than their batch, prior or not. */
typedef struct {
    int64_t prior_objects;          /* objects with a prior cluster */
    int64_t prior_representatives;  /* = prior clusters */
    int64_t joined_prior_cluster;   /* new genomes that joined a representative the prior named (the rest of joined_prior + joined_new joined a founder) */
} vg_derep_update_stats;
/* The array-level call.  g: any set; n_db: the number of database genomes in it (input ids 0 .. n_db - 1, as vg_genomes_load_db_new
 * returns it) -- checked against the set and otherwise not read: a database genome without a prior cluster is a new object like any
 * other.  prior_rep[n], indexed by object (rank): the object index of the representative of its prior cluster, or -1 = new, by the
 * rules of vg_cluster_update_graph.  Everything else as vg_dereplicate_set; ust may be NULL.  Refused with VG_EINVAL before any
 * device use: what vg_dereplicate_set refuses, n_db outside 0..n, a prior_rep value outside -1..n-1 or not its own representative. */
int vg_dereplicate_update_set(vg_genomes* g, int n_db, const vg_derep_params* p, const int32_t* prior_rep, int32_t* label, int32_t* representative,
                              vg_task** tasks, vg_pair_stat** stats_rows, int64_t* n_tasks, vg_derep_stats* st, vg_derep_update_stats* ust);
/* File to file: the genome set is the one of vg_genomes_load_db_new (the database, then the new genomes), and prior_path is a
 * clusters.tsv read against its ids exactly as vg_cluster_update reads one (by name; prior_is_repr: column 2 holds representative
 * ids; same VG_EINVAL messages).  clusters.tsv is byte for byte the file of vg_prefilter_new -> vg_align_new with that filter ->
 * vg_cluster_update(VG_CLUSTER_CDHIT) for a prior that covers the database.  p as for vg_dereplicate; the table's .ids.tsv is the
 * combined set's, and the representatives' FASTA needs one multi-FASTA file on each side (the database's records first).
 * verbosity >= 1 adds a second line, `Dereplicate update: ...`, with the counts of ust. */
int vg_dereplicate_update(const char* const* db_paths, int n_db, const char* const* new_paths, int n_new, const char* prior_path, int prior_is_repr,
                          const char* out_path, const vg_derep_file_params* p, vg_derep_update_stats* ust);

/* ------------------------------------------------------------------ deduplicate ------- */
/* The first stage: FASTA files -> one FASTA of the distinct sequences + a duplicates list, in place of mfasta-tool
 * (cmd_mfasta_deduplicate, vclust.py:810-866, run at vclust.py:1351); DESIGN.md section 10 is the contract.  A record's sequence is its lines
 * without white space (space, tab, CR, LF), over the IUPAC codes ACGTRYSWKMBDHVN and '-', case-insensitive.  Two records
 * are duplicates when the sequences are equal or one is the reverse complement of the other; the earliest record of a
 * group is kept. */
typedef struct {
    int gzip_level;             /* 0 = plain output; 1..9 = gzip members compressed at that level */
    int num_threads;            /* host threads (0 = the library's default) */
    int verbosity;              /* >= 1: one summary line on stderr */
} vg_dedup_params;
typedef struct {
    int64_t records;            /* records read */
    int64_t unique;             /* records kept */
    int64_t removed;            /* records - unique */
    int64_t reverse;            /* removed records equal to the reverse complement of the kept one only */
    int64_t rounds;             /* verification rounds on the device */
    int64_t collisions;         /* candidate members that differed from their candidate head (hash collisions) */
} vg_dedup_stats;
/* The whole stage, file to file.  prefixes: NULL or n_paths strings put in front of every header of that file's records.
 * A byte outside the alphabet is VG_EINVAL `<file>:<line>: '<c>' is not an IUPAC nucleotide code`, reported before any
 * kernel runs; 2^31 or more records is VG_EOVERFLOW.  out_path gets the kept records in input order (header line
 * prefixed, sequence lines verbatim); dup_path the header `representative<TAB>duplicate<TAB>strand` and one line per
 * removed record. */
int vg_deduplicate(const char* const* paths, int n_paths, const char* const* prefixes, const char* out_path,
                   const char* dup_path, const vg_dedup_params* p);
/* The array-level stage: n sequences, sequence i = ascii[offsets[i] .. offsets[i + 1]) (white space skipped).
 * representative[i]: the index of the earliest record equal to i or to its reverse complement (i for a kept record);
 * strand[i]: 0 if record i equals its representative, 1 if it equals only the representative's reverse complement.
 * stats may be NULL. */
int vg_dedup_seqs(const char* ascii, const int64_t* offsets, int64_t n, int32_t* representative, int8_t* strand,
                  vg_dedup_stats* stats);
/* Circular mode: with circular != 0, two records of the same length are also duplicates when one
 * is a rotation of the other or of the other's reverse complement, rot(X, s)[i] = X[(i + s) mod L].  strand is then 0 when
 * the record equals some rotation of its representative, 1 when it equals only rotations of the representative's reverse
 * complement; offset is the smallest s with record == rot(Y, s), Y the representative (strand 0) or its reverse complement
 * (strand 1).  The duplicates file gains a fourth column: `representative<TAB>duplicate<TAB>strand<TAB>offset`. */
typedef struct {
    int circular;               /* 0 = equal or reverse complement only; != 0 = up to rotation as well */
} vg_dedup_options;
/* vg_deduplicate / vg_dedup_seqs with options.  options == NULL or circular == 0: exactly the calls above (three-column
 * duplicates file), and offset (may then be NULL) is filled with 0.  In circular mode offset[n] is required. */
int vg_deduplicate_ex(const char* const* paths, int n_paths, const char* const* prefixes, const char* out_path,
                      const char* dup_path, const vg_dedup_params* p, const vg_dedup_options* options);
int vg_dedup_seqs_ex(const char* ascii, const int64_t* offsets, int64_t n, const vg_dedup_options* options,
                     int32_t* representative, int8_t* strand, int64_t* offset, vg_dedup_stats* stats);
/* test knob: keep only the low `bits` (0..128) bits of the sequence hash (forces collisions); 128 = the default */
void vg_dedup_set_hash_bits(int bits);
/* Terminal repeats: assemblers write a circular contig as the circle followed by a copy of its first
 * bases.  tr(X) of a record of L symbols is the largest t with min_repeat <= t <= L / 2 and X[0 : t) == X[L - t : L), 0 when
 * there is none (symbols compare literally, case ignored); circ(X) = X[0 : L - tr(X)).  The calls below are the circular mode
 * applied to the circles: records are duplicates when their circles have the same length and one is a rotation of the other
 * or of its reverse complement (raw lengths may differ); the earliest record of a group is kept; strand and offset are the
 * circular mode's over circles.  repeat[i] = tr(record i).  The output FASTA holds the kept records verbatim, repeat
 * included; the duplicates file has six columns:
 * `representative<TAB>duplicate<TAB>strand<TAB>offset<TAB>repeat<TAB>representative_repeat`.  min_repeat < 1 is VG_EINVAL;
 * the other errors are those of vg_deduplicate / vg_dedup_seqs.  offset[n] and repeat[n] are required. */
typedef struct {
    int64_t with_repeat;        /* records with a terminal repeat */
    int64_t repeat_symbols;     /* sum of tr over all records */
    int64_t candidates;         /* candidate repeats compared in full */
    int64_t equal;              /* candidates that were equal */
    int64_t batches;            /* compare batches */
} vg_dedup_repeat_stats;
/* the terminal-repeat pass alone: repeat[i] = tr(record i) */
int vg_dedup_terminal_repeats(const char* ascii, const int64_t* offsets, int64_t n, int64_t min_repeat, int64_t* repeat);
/* stats and repeat_stats may be NULL */
int vg_dedup_seqs_circular_tr(const char* ascii, const int64_t* offsets, int64_t n, int64_t min_repeat, int32_t* representative,
                              int8_t* strand, int64_t* offset, int64_t* repeat, vg_dedup_stats* stats,
                              vg_dedup_repeat_stats* repeat_stats);
int vg_deduplicate_circular_tr(const char* const* paths, int n_paths, const char* const* prefixes, const char* out_path,
                               const char* dup_path, const vg_dedup_params* p, int64_t min_repeat);
/* Contained mode: X is contained in Y when len X <= len Y and X is a contiguous substring of Y or
 * of revcomp(Y) (linear, no wrap-around; symbols compare literally).  A non-empty record is removed when a longer record
 * contains it, or an earlier record of the same length equals it or its reverse complement.  Its representative is the
 * longest kept record that contains it, the earliest of several; strand is 0 when it occurs in the representative, 1 when
 * only in the representative's reverse complement; offset is the smallest s with Y[s .. s + len) == record, Y the
 * representative (strand 0) or its reverse complement (strand 1).  Empty records are contained in nothing and form one
 * group.  The duplicates file has the four columns of the circular mode.  Errors are those of vg_deduplicate /
 * vg_dedup_seqs; offset[n] is required. */
typedef struct {
    int64_t passes;             /* index passes (container positions are indexed in bounded passes) */
    int64_t positions;          /* container positions indexed, all passes */
    int64_t hits;               /* indexed windows that start with a record's anchor, both strands */
    int64_t candidates;         /* hits that leave room for the record in a longer (or equal, earlier) record: compared in full */
    int64_t verified;           /* candidates that were equal */
    int64_t slices;             /* candidate launches (the hits are cut into slices of bounded size) */
} vg_dedup_contained_stats;
int vg_deduplicate_contained(const char* const* paths, int n_paths, const char* const* prefixes, const char* out_path,
                             const char* dup_path, const vg_dedup_params* p);
/* stats and contained_stats may be NULL; stats->rounds = passes, stats->collisions = candidates - verified */
int vg_dedup_seqs_contained(const char* ascii, const int64_t* offsets, int64_t n, int32_t* representative, int8_t* strand,
                            int64_t* offset, vg_dedup_stats* stats, vg_dedup_contained_stats* contained_stats);
/* test knobs of the contained mode: symbols of a record's anchor (1..16, default 16; short anchors flood the compare with
 * false candidates), and the most container positions indexed per pass (0 = the default, sized from the free HBM) */
void vg_dedup_set_anchor_symbols(int w);
void vg_dedup_set_index_positions(int64_t n);

/* ------------------------------------------------------------------ synthetic input --- */
/* Workload generator of SURVEY.md 8(d) (bench / test input; no reference call site: the reference ships no
 * generator).  Same draws as vclust_amd/synth.py (splitmix64, counter based), multithreaded.  The family plan
 * -- family index, members, ancestor length per family -- comes from the caller.  *codes_out (bases 0..3 of
 * all genomes) and *offsets_out (n_genomes + 1) are released with vg_free(). */
int vg_synth_plan(const int64_t* fam_idx, const int32_t* members, const int32_t* lengths, int64_t n_fam,
                  uint64_t seed, double p_lo, double p_hi, int n_indels, int n_threads,
                  uint8_t** codes_out, int64_t** offsets_out, int64_t* n_genomes);

/* ------------------------------------------------------------------ measurement ------- */
/* per-kernel HIP-event timing on the library's stream (bench.py's roofline leg) */
void vg_profile_enable(int on);
void vg_profile_reset(void);
/* returns number of kernels recorded; fills up to cap entries */
typedef struct { char name[48]; double total_ms; int64_t launches; double bytes; } vg_kernel_time;
int  vg_profile_get(vg_kernel_time* out, int cap);

#ifdef __cplusplus
}
#endif
#endif
