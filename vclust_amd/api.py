"""Thin Python layer over the C ABI: device residency, the integer kernels and the writers.

Used by the vclust-compatible front-end (vclust_amd/cli.py), bench.py and the parity tests.
Everything computational happens inside libvclust_gpu.so.
"""
import ctypes as C
import inspect

import numpy as np

from . import _lib
from ._lib import (ALIGN_FIELDS, ALIGN_OUTFMT, CLUSTER_ALGORITHMS, LINKAGE_ALGORITHMS, UPDATE_ALGORITHMS, ClusterStat, ClusterStats,  # noqa: F401
                   ClusterUpdateStats, CoverRunStats, CoverSegment, CoverStat, DedupStats, DerepStats, DerepUpdateStats, KernelTime, LinkageStats, MclParams, MclStats, PairCount,
                   PaintDonor, PaintRunStats, PaintSegment, PaintStat, PairStat, Region, Task, as_dict, check, lz_params, path, path_array, ptr)
# the whole-stage calls (vclust_amd/stages.py: no numpy)
from .stages import (DEFAULT_LZ, align, align_params, cluster, cluster_stats, cover, deduplicate as deduplicate_files, derep_params, dereplicate,  # noqa: F401
                     paint, prefilter)


def _dtype(ctype):
    """numpy's dtype for a ctypes scalar or struct (the library's record structs have no padding, and neither has the dtype)."""
    d = np.dtype(ctype)
    return np.dtype(d.descr) if d.names else d


PAIR_DTYPE, TASK_DTYPE, STAT_DTYPE, REGION_DTYPE, CLUSTER_STAT_DTYPE = (_dtype(t) for t in (PairCount, Task, PairStat, Region, ClusterStat))
COVER_STAT_DTYPE, COVER_SEGMENT_DTYPE = _dtype(CoverStat), _dtype(CoverSegment)
PAINT_STAT_DTYPE, PAINT_SEGMENT_DTYPE, PAINT_DONOR_DTYPE = _dtype(PaintStat), _dtype(PaintSegment), _dtype(PaintDonor)
LINKAGE_DTYPE = np.dtype([('node_a', '<i8'), ('node_b', '<i8'), ('similarity', '<f8'), ('size', '<i8'), ('object_a', '<i4'),
                          ('object_b', '<i4')])
AVERAGE_LINKAGE_DTYPE = np.dtype(LINKAGE_DTYPE.descr + [('sum', '<u8'), ('pairs', '<u8')])


def _input(x, ctype):
    """x as a contiguous array of `ctype` elements -> (pointer, length); the pointer keeps the array alive."""
    arr = np.ascontiguousarray(x, dtype=_dtype(ctype))
    return ptr(arr, ctype), len(arr)


def _filled(n, ctypes, call, guard=False):
    """The frame of a call that fills one entry per object: a zeroed array of n entries for each of `ctypes` -- of one entry for
    n = 0, so that the pointer is valid, and under `guard` for n >= 2^31, which the library refuses before it writes -- handed to
    `call` as pointers -> the first n entries of each."""
    size = 1 if guard and n >= 1 << 31 else max(n, 1)
    arrays = [np.zeros(size, dtype=_dtype(t)) for t in ctypes]
    call(*[ptr(a, t) for a, t in zip(arrays, ctypes)])
    return [a[:n] for a in arrays]


def version():
    return _lib.load().vg_version().decode()


def device_count():
    return _lib.load().vg_device_count()


def set_device(idx):
    check(_lib.load().vg_set_device(int(idx)))


class _LibOwned:
    """Releases a library-owned buffer (vg_free) when the numpy array that views it is collected."""
    __slots__ = ('_ptr', '_free')

    def __init__(self, ptr, free):
        self._ptr, self._free = ptr, free

    def __del__(self):
        try:
            self._free(self._ptr)
        except Exception:
            pass


def _take(ptr, n, dtype):
    """A library-owned array as a numpy array WITHOUT a copy: the array views the buffer, which is handed back to
    the library (vg_free) when the last view of it is gone."""
    lib = _lib.load()
    if n <= 0:
        if ptr:
            lib.vg_free(C.cast(ptr, C.c_void_p))
        return np.zeros(0, dtype=dtype)
    buf = (C.c_char * (n * dtype.itemsize)).from_address(C.addressof(ptr.contents))
    buf._owner = _LibOwned(C.cast(ptr, C.c_void_p), lib.vg_free)      # lives exactly as long as the buffer object
    return np.frombuffer(buf, dtype=dtype, count=n)


class GenomeSet:
    """A set of genomes held by the library (host packed + HBM resident)."""

    def __init__(self, handle):
        self._h = handle
        self._lib = _lib.load()

    @classmethod
    def load(cls, paths, multisample, n_threads=1):
        h = C.c_void_p()
        check(_lib.load().vg_genomes_load(path_array(paths), len(paths), int(bool(multisample)), int(n_threads), C.byref(h)))
        return cls(h)

    @classmethod
    def load_db_new(cls, db_paths, new_paths, multisample, n_threads=1):
        """-> (set, n_db): the genomes of db_paths (ids 0 .. n_db - 1) followed by those of new_paths, as one set.  multisample:
        one multi-FASTA on each side; otherwise one genome per file.  A name on both sides is an error."""
        h, n_db = C.c_void_p(), C.c_int()
        check(_lib.load().vg_genomes_load_db_new(path_array(db_paths), len(db_paths), path_array(new_paths), len(new_paths),
                                                 int(bool(multisample)), int(n_threads), C.byref(h), C.byref(n_db)))
        return cls(h), n_db.value

    @classmethod
    def from_codes(cls, codes, offsets, names=None):
        """codes: uint8 array (0..3 ACGT, >3 N); offsets: int64 array of n+1 entries."""
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(offsets) - 1
        nm = None
        if names is not None:
            nm = (C.c_char_p * n)(*[s.encode() for s in names])
        h = C.c_void_p()
        check(_lib.load().vg_genomes_from_codes(ptr(codes), ptr(offsets), n, nm, C.byref(h)))
        return cls(h)

    def close(self):
        if self._h:
            self._lib.vg_genomes_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return self._lib.vg_genomes_count(self._h)

    @property
    def total_len(self):
        return self._lib.vg_genomes_total_len(self._h)

    def lengths(self):
        out = np.zeros(len(self), dtype=np.int64)
        if len(self):
            check(self._lib.vg_genomes_lengths(self._h, ptr(out, C.c_int64)))
        return out

    def names(self):
        return [self._lib.vg_genomes_name(self._h, i).decode() for i in range(len(self))]

    def codes(self, idx):
        """Bases of genome idx as held on the host (0..3 = ACGT, 4 = N)."""
        out = np.empty(int(self.lengths()[idx]), dtype=np.uint8)
        check(self._lib.vg_genomes_codes(self._h, int(idx), ptr(out)))
        return out

    def to_device(self):
        check(self._lib.vg_genomes_to_device(self._h))

    def subset(self, ids):
        """The genomes `ids` of this resident set, in that order, as a new set gathered on the device (vg_genomes_subset): no base
        travels from the host.  An id outside the set or listed twice, and a set that is not resident, are errors."""
        h = C.c_void_p()
        check(self._lib.vg_genomes_subset(self._h, *_input(ids, C.c_int32), C.byref(h)))
        return GenomeSet(h)

    def extend(self, parent, ids):
        """Append the genomes `ids` of `parent`, in that order, behind the last genome of this set, in place (vg_genomes_extend).  This
        set must be a subset() of that very parent (it may be empty).  Only the appended genomes are written; the genomes already
        here are neither read nor copied, unless the buffers have to grow (reserve() avoids that).  An id outside the parent, listed
        twice or in this set already is an error."""
        check(self._lib.vg_genomes_extend(self._h, parent._h, *_input(ids, C.c_int32)))

    def truncate(self, n):
        """Drop every genome from n on, in place (vg_genomes_truncate): what is left is, to every kernel, the subset() of the kept
        genomes.  The capacity stays."""
        check(self._lib.vg_genomes_truncate(self._h, int(n)))

    def reserve(self, bases, genomes):
        """Room for `genomes` genomes of `bases` bases in all (vg_genomes_reserve; padding is added by the call), so that extend()
        up to there never moves the set."""
        check(self._lib.vg_genomes_reserve(self._h, int(bases), int(genomes)))

    def dereplicate_set(self, batch_genomes=None, k=25, kmers_fraction=1.0, min_kmers=20, min_ident=0.7, lz=None, algorithm='cd-hit',
                        metric='tani', num_alns=0, want_rows=False, n_db=0, prior_rep=None, **mins):
        """Greedy clustering against representatives only (vg_dereplicate_set): the result of kmer_shared ->
        filter_pairs -> lz_align -> cluster_graph('cd-hit') on the rows that pass the filters as ani.tsv prints them, computed batch
        by batch against the representatives found so far.  mins: tani=, gani=, ani=, qcov=, rcov=, len_ratio=; the metric's must be
        above 0.  -> (label int32[n], representative int32[n], stats dict), indexed by rank (align_order); with want_rows=True also
        (tasks, stats rows) of every aligned ordered pair, in input-order ids, as write_ani takes them.
        prior_rep (one entry per rank: the rank of the representative of its prior cluster, -1 = new) adds the other genomes to
        that clustering (vg_dereplicate_update_set): the result of cluster_update_graph('cd-hit') with that prior, with only the
        prior representatives ever compared; n_db is the number of database genomes of a load_db_new set.  The stats then also
        hold prior_objects, prior_representatives and joined_prior_cluster."""
        prm = derep_params(batch_genomes, k, kmers_fraction, min_kmers, min_ident, lz, algorithm, metric, num_alns, mins)
        n = len(self)
        update = prior_rep is not None or bool(n_db)
        st, ust = DerepStats(), DerepUpdateStats()
        tp, sp, nt = C.POINTER(Task)(), C.POINTER(PairStat)(), C.c_int64()
        rows = [C.byref(x) if want_rows else None for x in (tp, sp, nt)]
        if update:
            prior, n_prior = _input(np.full(n, -1) if prior_rep is None else prior_rep, C.c_int32)
            if n_prior != n:
                raise ValueError('prior_rep must have one entry per genome')

        def call(lp, rp):
            if update:
                check(self._lib.vg_dereplicate_update_set(self._h, int(n_db), C.byref(prm), prior, lp, rp, *rows, C.byref(st), C.byref(ust)))
            else:
                check(self._lib.vg_dereplicate_set(self._h, C.byref(prm), lp, rp, *rows, C.byref(st)))
        label, rep = _filled(n, (C.c_int32, C.c_int32), call)
        stats = as_dict(st, ust) if update else as_dict(st)
        if not want_rows:
            return label, rep, stats
        return label, rep, stats, (_take(tp, nt.value, TASK_DTYPE), _take(sp, nt.value, STAT_DTYPE))

    # ---------------------------------------------------------------- prefilter
    def kmer_shared(self, k=25, fraction=1.0, shard=0, n_shards=1, min_shared=1):
        """-> (set_sizes int64[n], pairs structured array a>b with shared counts)."""
        pp, npairs = C.POINTER(PairCount)(), C.c_int64()
        sizes, = _filled(len(self), (C.c_int64,), lambda sp: check(self._lib.vg_kmer_shared(
            self._h, k, float(fraction), shard, n_shards, int(min_shared), sp, C.byref(pp), C.byref(npairs))))
        return sizes, _take(pp, npairs.value, PAIR_DTYPE)

    def kmer_shared_new(self, n_db, k=25, fraction=1.0, min_shared=1):
        """New genomes (ids n_db .. n - 1) against a database (ids 0 .. n_db - 1): kmer_shared restricted to the pairs a > b with
        a >= n_db.  set_sizes are -1 for the database genomes that no returned pair names."""
        pp, npairs = C.POINTER(PairCount)(), C.c_int64()
        sizes, = _filled(len(self), (C.c_int64,), lambda sp: check(self._lib.vg_kmer_shared_new(
            self._h, int(n_db), k, float(fraction), int(min_shared), sp, C.byref(pp), C.byref(npairs))))
        return sizes, _take(pp, npairs.value, PAIR_DTYPE)

    def kmer_geometry(self, k=25, fraction=1.0, shard=0, n_shards=1):
        """The index geometry of the first pass of kmer_shared with these arguments (vg_kmer_geometry; host only) -> dict of the
        fields of vg_kmer_geometry_info.  Only accepted, P and n_passes mean anything unless accepted == 1."""
        info = _lib.KmerGeometry()
        check(self._lib.vg_kmer_geometry(self._h, int(k), float(fraction), int(shard), int(n_shards), C.byref(info)))
        return as_dict(info)

    def kmer_level2_slots(self, k=25, fraction=1.0, shard=0, n_shards=1):
        """How level 2 of the first pass of kmer_shared with these arguments runs (vg_kmer_level2_slots; host only): record slots per
        final bucket of the one-pass form, or 0 = the counted level 2."""
        slots = C.c_int(0)
        check(self._lib.vg_kmer_level2_slots(self._h, int(k), float(fraction), int(shard), int(n_shards), C.byref(slots)))
        return int(slots.value)

    def kmer_set(self, idx, k=25, fraction=1.0):
        p = C.POINTER(C.c_uint64)()
        n = C.c_int64()
        check(self._lib.vg_kmer_set(self._h, idx, k, float(fraction), C.byref(p), C.byref(n)))
        return _take(p, n.value, np.dtype('<u8'))

    def filter_pairs(self, set_sizes, pairs, k=25, min_kmers=20, min_ident=0.7):
        """The pairs write_fltr would print (thresholds on shared count and ani-shorter), in memory."""
        out, n = C.POINTER(PairCount)(), C.c_int64()
        check(self._lib.vg_filter_pairs(int(k), int(min_kmers), float(min_ident), *_input(set_sizes, C.c_int64), *_input(pairs, PairCount),
                                        C.byref(out), C.byref(n)))
        return _take(out, n.value, PAIR_DTYPE)

    def write_fltr(self, out_path, set_sizes, pairs, k=25, fraction=1.0, min_kmers=20, min_ident=0.7, max_seqs=0):
        check(self._lib.vg_write_fltr(self._h, k, float(fraction), int(min_kmers), float(min_ident), int(max_seqs),
                                      _input(set_sizes, C.c_int64)[0], *_input(pairs, PairCount), path(out_path)))

    # ---------------------------------------------------------------- align
    def align_order(self):
        order, = _filled(len(self), (C.c_int32,), lambda p: check(self._lib.vg_align_order(self._h, p)))
        return order

    def read_filter(self, path=None, threshold=0.0):
        pp = C.POINTER(PairCount)()
        n = C.c_int64()
        check(self._lib.vg_read_filter(self._h, _lib.path(path or None), float(threshold), C.byref(pp), C.byref(n)))
        return _take(pp, n.value, PAIR_DTYPE)

    def align_tasks(self, pairs):
        tp, n = C.POINTER(Task)(), C.c_int64()
        check(self._lib.vg_align_tasks(self._h, *_input(pairs, PairCount), C.byref(tp), C.byref(n)))
        return _take(tp, n.value, TASK_DTYPE)

    def lz_prepare(self, pairs, lz=None):
        """Optional head start of lz_align: the indexes of the pairs' genomes are queued on the device now (they are built
        while align_tasks runs on the host); lz_align takes them over when its tasks name the same references."""
        check(self._lib.vg_lz_prepare(self._h, *_input(pairs, PairCount), C.byref(lz_params(lz))))

    def lz_align(self, tasks, lz=None, want_regions=False):
        """LZ parse of the ordered pairs -> stats (and regions)."""
        tp, n = _input(tasks, Task)
        rp, nr = C.POINTER(Region)(), C.c_int64()
        stats, = _filled(n, (PairStat,), lambda sp: check(self._lib.vg_lz_align(
            self._h, tp, n, C.byref(lz_params(lz)), sp, C.byref(rp) if want_regions else None, C.byref(nr))))
        if want_regions:
            return stats, _take(rp, nr.value, REGION_DTYPE)
        return stats

    def lz_index_dump(self, idx, lz=None):
        """The index lz_align would build for genome idx (parity tests) -> dict(bucket_end uint32[4^msl], entries uint32[n],
        pos_bits, tag_bits, path: 0..5 register build of 24..4 trips, 6 mid, 7 lds, 8 global)."""
        prm = lz_params(lz)
        tb, en = C.POINTER(C.c_uint32)(), C.POINTER(C.c_uint32)()
        n, pb, tg, path = C.c_int64(), C.c_int(), C.c_int(), C.c_int()
        check(self._lib.vg_lz_index_dump(self._h, int(idx), C.byref(prm), C.byref(tb), C.byref(en), C.byref(n),
                                         C.byref(pb), C.byref(tg), C.byref(path)))
        u4 = np.dtype('<u4')
        return dict(bucket_end=_take(tb, 1 << (2 * prm.msl), u4), entries=_take(en, n.value, u4),
                    pos_bits=pb.value, tag_bits=tg.value, path=path.value)

    def write_ani(self, out_path, tasks, stats, regions=None, columns=None, out_aln=None, lz=None,
                  out_filters=None, num_threads=0):
        tp, n = _input(tasks, Task)
        # (is_multifasta=False: this call has always left that field of vg_align_params 0)
        p = align_params(list(columns or ALIGN_OUTFMT['standard']), out_aln=out_aln, lz=lz, out_filters=out_filters, num_threads=int(num_threads),
                         is_multifasta=False)
        reg_ptr, nreg = _input(regions, Region) if regions is not None else (None, 0)
        check(self._lib.vg_write_ani(self._h, tp, _input(stats, PairStat)[0], n, reg_ptr, nreg, path(out_path), C.byref(p)))


def cluster_graph(n_objects, q, r, w, algorithm='single'):
    """Cluster n_objects objects linked by the rows (q[i], r[i]) of weight w[i] (vg_cluster_graph): self rows are dropped,
    duplicate and reverse rows merged to the maximum weight.  -> (label int32[n], representative int32[n], stats dict):
    label is the numbering of clusters.tsv, representative the index of each cluster's earliest member.  algorithm: one of
    CLUSTER_ALGORITHMS, or 'complete' -- the complete-linkage hierarchy after every merge (each cluster a clique of the rows)."""
    known = {**CLUSTER_ALGORITHMS, **LINKAGE_ALGORITHMS}
    if algorithm not in known:
        raise ValueError(f'algorithm {algorithm!r} is not computed by the library (choices: {", ".join(known)})')
    rows, n, st = _rows(q, r, w), int(n_objects), ClusterStats()
    label, rep = _filled(n, (C.c_int32, C.c_int32), lambda lp, rp: check(_lib.load().vg_cluster_graph(
        n, *rows, known[algorithm], lp, rp, C.byref(st))))
    return label, rep, as_dict(st)


def cluster_mcl_graph(n_objects, q, r, w, inflation=2.0, prune=1e-4, max_row=128, chaos_eps=1e-3, max_iterations=100, matrix=False):
    """Markov clustering of the graph of cluster_graph (vg_cluster_mcl_graph; DESIGN.md section 9, "Markov clustering"): weights in
    [0, 1]; the flow matrix is held in integers of 2^-30, so the result is the same on every run.  inflation: a multiple of 0.5 in
    [1.5, 6]; prune: entries below that share of a row are dropped; max_row: entries a row keeps at most; the run stops when the
    chaos of an iteration is <= chaos_eps, or after max_iterations (stats['converged'] == 0: there is a result all the same).
    -> (label int32[n], representative int32[n], stats dict), and with matrix=True also (offsets int64[n + 1], columns int32[nnz],
    values uint32[nnz]): the last matrix as CSR, columns ascending per row -- with max_iterations=t the iterate after t steps."""
    rows, n, st = _rows(q, r, w), int(n_objects), MclStats()
    prm = MclParams(float(inflation), float(prune), float(chaos_eps), int(max_row), int(max_iterations))
    off, col, val = C.POINTER(C.c_int64)(), C.POINTER(C.c_int32)(), C.POINTER(C.c_uint32)()
    csr = [C.byref(x) if matrix else None for x in (off, col, val)]
    label, rep = _filled(n, (C.c_int32, C.c_int32), lambda lp, rp: check(_lib.load().vg_cluster_mcl_graph(
        n, *rows, C.byref(prm), lp, rp, *csr, C.byref(st))), guard=True)
    stats = as_dict(st)
    if not matrix:
        return label, rep, stats
    nnz = int(stats['nnz'])
    return label, rep, stats, (_take(off, n + 1, np.dtype('<i8')), _take(col, nnz, np.dtype('<i4')), _take(val, nnz, np.dtype('<u4')))


def cluster_mcl_set_table_slots(slots=0):
    """Test knob (vg_cluster_mcl_set_table_slots): the LDS table slots a row of the Markov clustering may use; rows whose candidate
    bound exceeds them, and whose distinct columns fill more than 3/4 of them, take the spill path.  0 = the default."""
    _lib.load().vg_cluster_mcl_set_table_slots(int(slots))


def cluster_update_graph(n_objects, q, r, w, prior_rep, algorithm='single'):
    """Add new objects to a prior clustering (vg_cluster_update_graph; DESIGN.md section 9, "Update of a prior clustering").
    prior_rep[i] is -1 for a new object, else the index of the representative of i's prior cluster (its own representative; it
    need not be the cluster's earliest member).  Rows are read as by cluster_graph, and a row between two prior objects is
    ignored.  'cd-hit' / 'uclust': prior clusters and their representatives are frozen, and the new objects are visited after
    the prior ones; 'single': the components of the prior partition plus the kept rows.  -> (label int32[n], representative
    int32[n], stats dict): label numbers the final partition by earliest member, representative is the frozen or founding
    representative (single: the earliest member)."""
    if algorithm not in UPDATE_ALGORITHMS:
        raise ValueError(f'algorithm {algorithm!r} cannot update a prior clustering (choices: {", ".join(UPDATE_ALGORITHMS)})')
    rows, n, st = _rows(q, r, w), int(n_objects), ClusterUpdateStats()
    prior, n_prior = _input(prior_rep, C.c_int32)
    if n < 1 << 31 and n_prior != n:
        raise ValueError('prior_rep must have one entry per object')
    label, rep = _filled(n, (C.c_int32, C.c_int32), lambda lp, rp: check(_lib.load().vg_cluster_update_graph(
        n, *rows, UPDATE_ALGORITHMS[algorithm], prior, lp, rp, C.byref(st))), guard=True)
    return label, rep, as_dict(st)


def cluster_update(ani_path, ids_path, prior_path, out_path, algorithm='single', prior_repr=False, **options):
    """clusters.tsv of the objects of the ids file, with the clusters of the clusters.tsv `prior_path` taken as given
    (vg_cluster_update).  prior_repr: the second column of prior_path holds representative ids (as representatives=True writes
    them).  options: those of cluster().  -> the update's counts as a dict."""
    return cluster(ani_path, ids_path, out_path, algorithm=algorithm, prior_path=prior_path, prior_repr=prior_repr, **options)


def cluster_stats_graph(n_objects, q, r, w, label, n_clusters=None):
    """The cluster report of the labelling label[i] in [0, n_clusters) on the graph of cluster_graph (vg_cluster_stats_graph; DESIGN.md
    section 9, "Cluster report"): weights in [0, 1], taken as u = round(w * 2^32).  n_clusters: default max(label) + 1.  ->
    (records CLUSTER_STAT_DTYPE[n_clusters], own_max uint64[n], other_max uint64[n], other int32[n]); every figure is an integer."""
    rows, n = _rows(q, r, w), int(n_objects)
    label = np.ascontiguousarray(label, dtype=np.int32)
    if n < 1 << 31 and len(label) != n:
        raise ValueError('label must have one entry per object')
    if n_clusters is None:
        n_clusters = int(label.max()) + 1 if len(label) else 0
    k = int(n_clusters)
    out = np.zeros(max(k, 1) if 0 <= k < 1 << 31 else 1, dtype=CLUSTER_STAT_DTYPE)
    own, oth, lab = _filled(n, (C.c_uint64, C.c_uint64, C.c_int32), lambda *per_object: check(_lib.load().vg_cluster_stats_graph(
        n, *rows, ptr(label, C.c_int32), k, ptr(out, ClusterStat), *per_object)), guard=True)
    return out[:k], own, oth, lab


def cover_rows(lengths, q, r, qstart, qend, label=None, n_groups=None, segments=True):
    """The coverage map of the rows (q[i], r[i], qstart[i], qend[i]) -- positions qstart..qend (0-based, inclusive) of object q are
    aligned to partner r -- over objects of the given lengths (vg_cover_rows).  label[i] in [0, n_groups):
    the groups that split the depth into `in` and `out` (default: one group; n_groups: default max(label) + 1).  ->
    (records COVER_STAT_DTYPE[n], segments COVER_SEGMENT_DTYPE[...] or None with segments=False, run_stats dict)."""
    lp, n = _input(lengths, C.c_int64)
    (qp, nq), (rp, nr), (sp, ns), (ep, ne) = _input(q, C.c_uint32), _input(r, C.c_uint32), _input(qstart, C.c_int32), _input(qend, C.c_int32)
    if not nq == nr == ns == ne:
        raise ValueError('q, r, qstart and qend must have the same length')
    gp, k = None, 0
    if label is not None:
        label = np.ascontiguousarray(label, dtype=np.int32)
        if len(label) != n:
            raise ValueError('label must have one entry per object')
        gp, k = ptr(label, C.c_int32), int(n_groups) if n_groups is not None else (int(label.max()) + 1 if n else 1)
    elif n_groups is not None:
        raise ValueError('n_groups needs label')
    seg, n_seg, st = C.POINTER(CoverSegment)(), C.c_int64(), CoverRunStats()
    records, = _filled(n, (CoverStat,), lambda out: check(_lib.load().vg_cover_rows(
        n, lp, gp, k, qp, rp, sp, ep, nq, out, C.byref(seg) if segments else None, C.byref(n_seg) if segments else None, C.byref(st))))
    return records, _take(seg, n_seg.value, COVER_SEGMENT_DTYPE) if segments else None, as_dict(st)


def cover_regions(genomes, tasks, regions, label=None):
    """The coverage map of a run without any file: `tasks` (TASK_DTYPE) and `regions` (REGION_DTYPE) as GenomeSet.lz_align takes
    and returns them over the GenomeSet `genomes`; a region is a row (q, r) of its task with its qstart, qend.  -> as cover_rows."""
    tasks, regions = np.asarray(tasks), np.asarray(regions)
    t = regions['task']
    return cover_rows(genomes.lengths(), tasks['q'][t], tasks['r'][t], regions['qstart'], regions['qend'], label=label)


def paint_rows(lengths, q, r, qstart, qend, n_match, label=None, n_groups=None, segments=True, donors=True):
    """The mosaic painting of the rows (q[i], r[i], qstart[i], qend[i], n_match[i]) -- positions qstart..qend (0-based, inclusive) of
    object q are aligned to partner r with n_match matching positions -- over objects of the given lengths (vg_paint_rows; DESIGN.md
    section 15): at every position the covering row of the highest identity wins.  label, n_groups: as in cover_rows; they split the
    painted positions into `in` and `out`.  -> (records PAINT_STAT_DTYPE[n], segments PAINT_SEGMENT_DTYPE[...] or None with
    segments=False, donor records PAINT_DONOR_DTYPE[...] or None with donors=False, run_stats dict)."""
    lp, n = _input(lengths, C.c_int64)
    (qp, nq), (rp, nr), (sp, ns), (ep, ne), (mp, nm) = (_input(q, C.c_uint32), _input(r, C.c_uint32), _input(qstart, C.c_int32), _input(qend, C.c_int32),
                                                        _input(n_match, C.c_int32))
    if not nq == nr == ns == ne == nm:
        raise ValueError('q, r, qstart, qend and n_match must have the same length')
    gp, k = None, 0
    if label is not None:
        label = np.ascontiguousarray(label, dtype=np.int32)
        if len(label) != n:
            raise ValueError('label must have one entry per object')
        gp, k = ptr(label, C.c_int32), int(n_groups) if n_groups is not None else (int(label.max()) + 1 if n else 1)
    elif n_groups is not None:
        raise ValueError('n_groups needs label')
    seg, n_seg, don, n_don, st = C.POINTER(PaintSegment)(), C.c_int64(), C.POINTER(PaintDonor)(), C.c_int64(), PaintRunStats()
    records, = _filled(n, (PaintStat,), lambda out: check(_lib.load().vg_paint_rows(
        n, lp, gp, k, qp, rp, sp, ep, mp, nq, out, C.byref(seg) if segments else None, C.byref(n_seg) if segments else None,
        C.byref(don) if donors else None, C.byref(n_don) if donors else None, C.byref(st))))
    return (records, _take(seg, n_seg.value, PAINT_SEGMENT_DTYPE) if segments else None,
            _take(don, n_don.value, PAINT_DONOR_DTYPE) if donors else None, as_dict(st))


def paint_regions(genomes, tasks, regions, label=None):
    """The mosaic painting of a run without any file: tasks and regions as in cover_regions; a region is a row (q, r) of its task with
    its qstart, qend and n_match.  -> as paint_rows."""
    tasks, regions = np.asarray(tasks), np.asarray(regions)
    t = regions['task']
    return paint_rows(genomes.lengths(), tasks['q'][t], tasks['r'][t], regions['qstart'], regions['qend'], regions['n_match'], label=label)


def _rows(q, r, w):
    """The rows of a graph as the array-level calls take them -> (q pointer, r pointer, w pointer, number of rows)."""
    (q, n), (r, nr), (w, nw) = _input(q, C.c_uint32), _input(r, C.c_uint32), _input(w, C.c_double)
    if not n == nr == nw:
        raise ValueError('q, r and w must have the same length')
    return q, r, w, n


def _linkage_table(fn, n_objects, q, r, w, floor=None):
    """-> (table, stats) of the array-level merge-table call `fn`.  With a floor, `fn` is the average-linkage entry: it takes the
    floor after the rows and returns `sum` and `pairs` after the similarity, in an AVERAGE_LINKAGE_DTYPE table."""
    rows, n = _rows(q, r, w), int(n_objects)
    cap = max(n - 1, 1) if n < 1 << 31 else 1          # (2^31 objects or more: the library refuses before it writes)
    # object_a, object_b, similarity, (sum, pairs,) node_a, node_b, size: one entry per merge, in the order of the C arguments
    ctypes = (C.c_int32, C.c_int32, C.c_double) + (() if floor is None else (C.c_uint64, C.c_uint64)) + (C.c_int64,) * 3
    arrays = [np.zeros(cap, dtype=t) for t in ctypes]
    nm, st = C.c_int64(0), LinkageStats()
    check(getattr(_lib.load(), fn)(n, *rows, *([] if floor is None else [float(floor)]), *[ptr(a, t) for a, t in zip(arrays, ctypes)],
                                   C.byref(nm), C.byref(st)))
    oa, ob, wt, *exact, na, nb, sz = arrays
    table = np.zeros(nm.value, dtype=LINKAGE_DTYPE if floor is None else AVERAGE_LINKAGE_DTYPE)
    for name, arr in zip(table.dtype.names, (na, nb, wt, sz, oa, ob, *exact)):
        table[name] = arr[:nm.value]
    return table, as_dict(st)


def cluster_linkage(n_objects, q, r, w):
    """The single-linkage merge table of the graph of cluster_graph (vg_cluster_linkage_graph): the maximum spanning forest in
    the order (similarity descending, object_a, object_b).  -> (table, stats): table is a LINKAGE_DTYPE array with one record
    per merge -- merge k creates node n_objects + k from node_a < node_b and has `size` members; (object_a, object_b,
    similarity) is the edge -- and stats a dict(rounds, n_edges, n_merges)."""
    return _linkage_table('vg_cluster_linkage_graph', n_objects, q, r, w)


def cluster_complete_linkage_graph(n_objects, q, r, w):
    """The complete-linkage merge table of the graph of cluster_graph (vg_cluster_complete_linkage_graph).  K(A, B) of two clusters
    is the worst edge between them in the order (similarity descending, object_a, object_b), infinite when any pair of their
    members has no edge; from singletons, the two clusters of smallest finite K merge until none is left, so every cluster is a
    clique of the rows.  -> (table, stats) as cluster_linkage: (object_a, object_b, similarity) is that worst edge, `similarity`
    never rises down the table, and stats['rounds'] counts the parallel merge rounds."""
    return _linkage_table('vg_cluster_complete_linkage_graph', n_objects, q, r, w)


def cluster_complete_levels_graph(n_objects, q, r, w, levels):
    """The cuts of one complete-linkage merge table at `levels` (vg_cluster_complete_levels_graph): the cut at t joins the merges
    of similarity >= t and equals cluster_graph(rows with w >= t, 'complete'); every cluster of it is a clique of those rows and
    lies inside one cluster of cluster_levels at t.  -> as cluster_levels."""
    return _levels('vg_cluster_complete_levels_graph', n_objects, q, r, w, levels)


def cluster_average_linkage_graph(n_objects, q, r, w, floor=0.0):
    """The average-linkage (UPGMA) merge table of the graph of cluster_graph (vg_cluster_average_linkage_graph), in exact integer
    arithmetic: a weight (in [0, 1]) is u = round(w * 2^32), sim(A, B) = S / (|A| |B| 2^32) with S the sum of u over the rows
    between the two clusters (a pair without a row counts as 0; two clusters without any row between them never merge), and from
    singletons the pair of smallest key (-sim, c, d) merges until none is left or sim < floor.  -> (table, stats): table is an
    AVERAGE_LINKAGE_DTYPE array -- the fields of cluster_linkage with (object_a, object_b) the two cluster ids merged, plus the
    exact `sum` S and `pairs` P = |A| |B| of each record; `similarity` is the double nearest to S / (P 2^32) and never rises."""
    return _linkage_table('vg_cluster_average_linkage_graph', n_objects, q, r, w, floor)


def cluster_average_levels_graph(n_objects, q, r, w, levels, floor=0.0):
    """The cuts of one average-linkage merge table at `levels` (vg_cluster_average_levels_graph): the cut at t joins the merges
    with S >= round(t * 2^32) * P, compared exactly.  No level may lie below `floor`.  It is NOT cluster_average_linkage_graph
    with floor t cut at its floor: the rows between floor and t still count in the averages.  -> as cluster_levels."""
    return _levels('vg_cluster_average_levels_graph', n_objects, q, r, w, levels, floor)


def cluster_average_similarity(s, p):
    """Test entry (vg_cluster_average_similarity): the double nearest to s / (p * 2^32), ties to even."""
    return float(_lib.load().vg_cluster_average_similarity(int(s), int(p)))


def cluster_average_order_selftest(s, size_c, size_d, c, d, on_device=False):
    """Test entry (vg_cluster_average_order_selftest): the shared comparator of average linkage over neighbouring entries ->
    int8[n - 1] of -1 / 0 / 1, entry i against entry i + 1 (smaller key = larger s / (size_c * size_d), then smaller (c, d))."""
    (s, n), arrs = _input(s, C.c_uint64), [_input(x, C.c_uint32) for x in (size_c, size_d, c, d)]
    if any(nx != n for _, nx in arrs):
        raise ValueError('the five arrays must have the same length')
    out, = _filled(n - 1, (C.c_int8,), lambda op: check(_lib.load().vg_cluster_average_order_selftest(
        s, *[x for x, _ in arrs], n, int(bool(on_device)), op)))
    return out


def cluster_levels(n_objects, q, r, w, levels):
    """The cuts of one merge table at `levels` (vg_cluster_levels_graph): the cut at t joins the merges of similarity >= t and
    equals cluster_graph(rows with w >= t, 'single').  -> (label int32[len(levels), n], representative int32[len(levels), n],
    stats dict), rows in the order of the levels."""
    return _levels('vg_cluster_levels_graph', n_objects, q, r, w, levels)


def _levels(fn, n_objects, q, r, w, levels, floor=None):
    """-> (label, representative, stats) of the array-level cuts call `fn`; with a floor, of the average-linkage entry"""
    rows, n = _rows(q, r, w), int(n_objects)
    lv, n_levels = _input(np.reshape(levels, -1), C.c_double)
    width = n if 0 < n < 1 << 31 else 1                # (the library's row stride is n; it writes nothing otherwise)
    label = np.zeros((n_levels, width), dtype=np.int32)
    rep = np.zeros((n_levels, width), dtype=np.int32)
    st = LinkageStats()
    check(getattr(_lib.load(), fn)(n, *rows, *([] if floor is None else [float(floor)]), lv, n_levels, ptr(label, C.c_int32), ptr(rep, C.c_int32),
                                   C.byref(st)))
    return label[:, :n], rep[:, :n], as_dict(st)


def _seq_buffer(seqs):
    """-> (the sequences back to back, int64 offsets[n + 1], n)"""
    bufs = [s.encode() if isinstance(s, str) else bytes(s) for s in seqs]
    n = len(bufs)
    offsets = np.zeros(n + 1, dtype=np.int64)
    if n:
        offsets[1:] = np.cumsum([len(b) for b in bufs])
    return b''.join(bufs), offsets, n


def terminal_repeats(seqs, min_repeat):
    """The terminal repeat of every sequence (vg_dedup_terminal_repeats) -> int64[n]: the largest t with
    min_repeat <= t <= len // 2 whose first t symbols equal its last t symbols (literally, case ignored), 0 without one."""
    ascii, offsets, n = _seq_buffer(seqs)
    repeat, = _filled(n, (C.c_int64,), lambda rp: check(_lib.load().vg_dedup_terminal_repeats(
        ascii, ptr(offsets, C.c_int64), n, int(min_repeat), rp)))
    return repeat


def deduplicate(seqs, circular=False, contained=False, **options):
    """Group the sequences `seqs` (str or bytes each; white space is skipped, case ignored) by equality up to reverse
    complement (vg_dedup_seqs).  -> (representative int32[n], strand int8[n], stats dict): representative[i] is the index of
    the earliest sequence of i's group, strand[i] is 1 when i equals only that sequence's reverse complement, else 0.
    circular=True (vg_dedup_seqs_ex): rotations of a sequence and of its reverse complement are equal too; strand[i] is 1
    when i equals only rotations of the reverse complement, and the result is (representative, strand, offset int64[n],
    stats) with offset[i] the smallest s for which i == rot(representative or its reverse complement, s).
    contained=True (vg_dedup_seqs_contained): a sequence that is a substring of a longer one, or of its reverse complement,
    is removed too; representative[i] is the longest kept sequence that contains i (the earliest of several), strand[i] is 1
    when i occurs only in its reverse complement, and the result is (representative, strand, offset int64[n], stats) with
    offset[i] the smallest position of i in the representative (strand 0) or its reverse complement (strand 1); stats also
    holds the counters of vg_dedup_contained_stats.  circular and contained together raise ValueError.
    circular=True, terminal_repeat=m (vg_dedup_seqs_circular_tr): an exact terminal repeat of at least m symbols (see
    terminal_repeats) is taken off every sequence first, and the circular result is that of the remaining circles;
    stats['repeat'] is the int64[n] array of the repeats, beside the counters of vg_dedup_repeat_stats.  terminal_repeat
    without circular raises ValueError."""
    unknown = set(options) - {'terminal_repeat'}
    if unknown:
        raise TypeError(f'deduplicate() got an unexpected keyword argument {sorted(unknown)[0]!r}')
    terminal_repeat = options.get('terminal_repeat')
    mode = _lib.dedup_mode(circular, contained, terminal_repeat is not None, needs='circular=True')
    ascii, offsets, n = _seq_buffer(seqs)
    st, more = DedupStats(), [mode.more_stats()] if mode.more_stats else []
    # representative, strand, and the mode's offsets and repeats
    arrays = _filled(n, (C.c_int32, C.c_int8) + (C.c_int64,) * mode.n_arrays, lambda *per_sequence: check(getattr(_lib.load(), mode.seqs)(
        ascii, ptr(offsets, C.c_int64), n, *mode.extra(terminal_repeat), *per_sequence, C.byref(st), *map(C.byref, more))))
    stats = as_dict(st, *more)
    if mode.n_arrays == 2:
        stats['repeat'] = arrays.pop()
    return (*arrays, stats)


# The introspected signature stays the three parameters of the plain, circular and contained modes, which
# tests/test_dedup_contained_cpu.py pins as the whole list; terminal_repeat is an option on top of them, accepted by keyword only.
deduplicate.__signature__ = inspect.Signature([p for p in inspect.signature(deduplicate).parameters.values()
                                               if p.kind is not inspect.Parameter.VAR_KEYWORD])


def dedup_set_hash_bits(bits=128):
    """Test knob (vg_dedup_set_hash_bits): keep only the low `bits` bits of the sequence hash; 128 = the default."""
    _lib.load().vg_dedup_set_hash_bits(int(bits))


def dedup_set_anchor_symbols(w=16):
    """Test knob (vg_dedup_set_anchor_symbols): symbols of an anchor in the contained mode, 1..16; 16 = the default."""
    _lib.load().vg_dedup_set_anchor_symbols(int(w))


def dedup_set_index_positions(n=0):
    """Test knob (vg_dedup_set_index_positions): container positions indexed per pass in the contained mode; 0 = the default."""
    _lib.load().vg_dedup_set_index_positions(int(n))


def set_lz_fit(weak_seed_ratio=3, anchor_margin=-1, seed_choice=3):
    """The three thin constants of the LZ restatement (vg_set_lz_fit); no arguments = the fitted values."""
    f = _lib.LzFit(int(weak_seed_ratio), int(anchor_margin), int(seed_choice))
    _lib.load().vg_set_lz_fit(C.byref(f))


def set_range_scan(mode):
    """0 = a RANGE shard call scans every base itself; 1 = the sliced scan of the multi-GPU path with the peers' slices
    computed by this process (vg_set_range_scan)."""
    _lib.load().vg_set_range_scan(int(mode))


def set_placement_trials(n):
    """Placements of the prefilter workspace the first dense pass of this process may try (vg_set_placement_trials; 1 = none, the default)."""
    _lib.load().vg_set_placement_trials(int(n))


def set_new_path(mode):
    """Route of GenomeSet.kmer_shared_new (vg_set_new_path): 0 = automatic, 1 = never the masked route, 2 = the masked route wherever
    it applies."""
    _lib.load().vg_set_new_path(int(mode))


def kmer_geometry_at(padded_positions, k=25):
    """GenomeSet.kmer_geometry for the dense single pass over a set of that many padded positions, without a set
    (vg_kmer_geometry_at)."""
    info = _lib.KmerGeometry()
    check(_lib.load().vg_kmer_geometry_at(int(padded_positions), int(k), C.byref(info)))
    return as_dict(info)


def rowptr_inline_lo(entries, n_genomes):
    """The smallest row-pointer value that carries a genome id in a prefilter pass of `entries` genome-list slots over `n_genomes`
    genomes, or 0 where such a pass inlines nothing (vg_rowptr_inline_lo; host only)."""
    lo = C.c_uint32(0)
    check(_lib.load().vg_rowptr_inline_lo(int(entries), int(n_genomes), C.byref(lo)))
    return int(lo.value)


def release_device_memory():
    _lib.load().vg_release_device_memory()


# ---------------------------------------------------------------- measurement
def profile_enable(on=True):
    _lib.load().vg_profile_enable(int(bool(on)))


def profile_reset():
    _lib.load().vg_profile_reset()


def profile_get():
    lib = _lib.load()
    arr = (KernelTime * 64)()
    n = lib.vg_profile_get(arr, 64)
    return [dict(name=arr[i].name.decode(), total_ms=arr[i].total_ms, launches=arr[i].launches,
                 bytes=arr[i].bytes) for i in range(min(n, 64))]
