"""ctypes binding of libvclust_gpu.so (include/vclust_gpu.h).

The library is the product: there is no Python or CPU fallback.  If the shared object is
missing the import fails loudly and tells how to build it.
"""
import collections
import ctypes as C
import os
import pathlib

PKG_DIR = pathlib.Path(__file__).resolve().parent
LIB_PATH = PKG_DIR / 'libvclust_gpu.so'


class VclustGpuError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f'libvclust_gpu error {code}: {msg}')
        self.code = code


class PairCount(C.Structure):
    _fields_ = [('a', C.c_uint32), ('b', C.c_uint32), ('shared', C.c_uint32)]


class Task(C.Structure):
    _fields_ = [('q', C.c_uint32), ('r', C.c_uint32)]


class PairStat(C.Structure):
    _fields_ = [('n_match', C.c_uint32), ('aln_len', C.c_uint32), ('n_regions', C.c_uint32)]


class Region(C.Structure):
    _fields_ = [('task', C.c_uint32), ('qstart', C.c_int32), ('qend', C.c_int32),
                ('rstart', C.c_int32), ('rend', C.c_int32), ('n_match', C.c_int32)]


class LzParams(C.Structure):
    _fields_ = [(n, C.c_int) for n in ('mal', 'msl', 'mrd', 'mqd', 'reg', 'aw', 'am', 'ar')]


DEFAULT_LZ = dict(mal=11, msl=7, mrd=40, mqd=40, reg=35, aw=15, am=7, ar=3)


def lz_params(lz=None):
    """vg_lz_params: DEFAULT_LZ, overridden by the entries of the dict `lz`."""
    return LzParams(**{**DEFAULT_LZ, **(lz or {})})


class LzFit(C.Structure):
    _fields_ = [('weak_seed_ratio', C.c_int), ('anchor_margin', C.c_int), ('seed_choice', C.c_int)]


class PrefilterParams(C.Structure):
    _fields_ = [('k', C.c_int), ('min_kmers', C.c_int), ('min_ident', C.c_double),
                ('batch_size', C.c_int), ('kmers_fraction', C.c_double), ('max_seqs', C.c_int),
                ('num_threads', C.c_int), ('verbosity', C.c_int), ('is_multifasta', C.c_int)]


# LZ-ANI output columns and the three output formats (same sets as the reference, vclust.py:38-47)
ALIGN_FIELDS = ['qidx', 'ridx', 'query', 'reference', 'tani', 'gani', 'ani', 'qcov', 'rcov',
                'num_alns', 'len_ratio', 'qlen', 'rlen', 'nt_match', 'nt_mismatch']
ALIGN_OUTFMT = {
    'lite': ALIGN_FIELDS[:2] + ALIGN_FIELDS[4:11],
    'standard': ALIGN_FIELDS[:11],
    'complete': ALIGN_FIELDS[:],
}


class AlignParams(C.Structure):
    _fields_ = [('lz', LzParams),
                ('out_tani', C.c_double), ('out_gani', C.c_double), ('out_ani', C.c_double),
                ('out_qcov', C.c_double), ('out_rcov', C.c_double),
                ('filter_path', C.c_char_p), ('filter_threshold', C.c_double),
                ('out_aln_path', C.c_char_p),
                ('out_columns', C.POINTER(C.c_char_p)), ('n_out_columns', C.c_int),
                ('num_threads', C.c_int), ('verbosity', C.c_int), ('is_multifasta', C.c_int)]


class ClusterParams(C.Structure):
    _fields_ = [('algorithm', C.c_int), ('metric', C.c_char_p),
                ('min_tani', C.c_double), ('min_gani', C.c_double), ('min_ani', C.c_double),
                ('min_qcov', C.c_double), ('min_rcov', C.c_double), ('min_len_ratio', C.c_double),
                ('max_num_alns', C.c_int), ('representatives', C.c_int), ('num_threads', C.c_int), ('verbosity', C.c_int)]


class DerepParams(C.Structure):
    """vg_derep_params: prefilter, align and cluster options of dereplicate, and its batch size"""
    _fields_ = [('k', C.c_int), ('kmers_fraction', C.c_double), ('min_kmers', C.c_int), ('min_ident', C.c_double), ('lz', LzParams),
                ('cluster', ClusterParams), ('batch_genomes', C.c_int)]


class DerepStats(C.Structure):
    _fields_ = [(name, C.c_int64) for name in ('batches', 'representatives', 'pairs_candidate', 'pairs_aligned', 'pairs_skipped',
                                                'joined_prior', 'joined_new', 'founded')]


class DerepUpdateStats(C.Structure):
    """vg_derep_update_stats: what dereplicate counts beside DerepStats when it adds genomes to an earlier run"""
    _fields_ = [(name, C.c_int64) for name in ('prior_objects', 'prior_representatives', 'joined_prior_cluster')]


class DerepFileParams(C.Structure):
    _fields_ = [('derep', DerepParams), ('representatives', C.c_int), ('out_table_path', C.c_char_p),
                ('out_columns', C.POINTER(C.c_char_p)), ('n_out_columns', C.c_int), ('out_repr_fasta_path', C.c_char_p),
                ('num_threads', C.c_int), ('verbosity', C.c_int), ('is_multifasta', C.c_int), ('stats', C.POINTER(DerepStats))]


class ClusterStats(C.Structure):
    _fields_ = [('rounds', C.c_int64), ('sweep_objects', C.c_int64), ('n_edges', C.c_int64)]


class ClusterUpdateStats(C.Structure):
    _fields_ = [(name, C.c_int64) for name in ('rounds', 'sweep_objects', 'n_edges', 'n_prior', 'n_new', 'joined_prior', 'joined_new',
                                                'founded', 'prior_merged')]


class ClusterStat(C.Structure):
    """vg_cluster_stat: the record of one cluster in the cluster report"""
    _fields_ = [('size', C.c_int64), ('rep', C.c_int64), ('pairs', C.c_uint64), ('linked', C.c_uint64), ('sum', C.c_uint64),
                ('min', C.c_uint64), ('external', C.c_uint64), ('nearest', C.c_int64), ('nearest_max', C.c_uint64),
                ('nearest_sum', C.c_uint64), ('misfits', C.c_int64)]


class CoverStat(C.Structure):
    """vg_cover_stat: the record of one object in the coverage map"""
    _fields_ = [(name, C.c_int64) for name in ('len', 'partners_in', 'partners_out', 'covered', 'covered_in', 'covered_out', 'core',
                                                'sum_in', 'sum_out', 'max_depth', 'segments')]


class CoverSegment(C.Structure):
    """vg_cover_segment: a maximal run of constant (depth_in, depth_out), positions 0-based inclusive"""
    _fields_ = [(name, C.c_int32) for name in ('object', 'start', 'end', 'depth_in', 'depth_out')]


class CoverRunStats(C.Structure):
    _fields_ = [(name, C.c_int64) for name in ('rows_kept', 'intervals', 'breakpoints', 'segments')]


class PaintStat(C.Structure):
    """vg_paint_stat: the record of one object in the mosaic painting"""
    _fields_ = [(name, C.c_int64) for name in ('len', 'painted', 'painted_in', 'painted_out', 'donors', 'top_partner', 'top_painted', 'switches',
                                                'segments')]


class PaintSegment(C.Structure):
    """vg_paint_segment: a maximal run of one winning row (partner -1: of no winner), positions 0-based inclusive"""
    _fields_ = [(name, C.c_int32) for name in ('object', 'start', 'end', 'partner', 'row_qstart', 'row_qend', 'n_match')]


class PaintDonor(C.Structure):
    """vg_paint_donor: what one winning partner paints of one object"""
    _fields_ = [('object', C.c_int32), ('partner', C.c_int32), ('painted', C.c_int64), ('segments', C.c_int64)]


class PaintRunStats(C.Structure):
    _fields_ = [(name, C.c_int64) for name in ('rows_kept', 'breakpoints', 'segments', 'donor_records', 'levels')]


class LinkageStats(C.Structure):
    _fields_ = [('rounds', C.c_int64), ('n_edges', C.c_int64), ('n_merges', C.c_int64)]


# --algorithm values the library clusters itself (VG_CLUSTER_*); complete / leiden stay with Clusty
CLUSTER_ALGORITHMS = {'single': 0, 'cd-hit': 1, 'uclust': 2, 'set-cover': 3}
# the hierarchies the library computes (merge table and cuts: --out-linkage / --levels); 'complete' is also an algorithm of
# vg_cluster / vg_cluster_graph (the cut at the floor), but a plain `cluster --algorithm complete` still goes to Clusty
LINKAGE_ALGORITHMS = {'single': 0, 'complete': 4}
# ... and with average linkage (UPGMA), which Clusty does not have: it always runs in the library, with or without the merge table
HIERARCHY_ALGORITHMS = {**LINKAGE_ALGORITHMS, 'average': 5}
# the algorithms under which new objects are added to a prior clustering (vg_cluster_update / vg_cluster_update_graph)
UPDATE_ALGORITHMS = {'single': 0, 'cd-hit': 1, 'uclust': 2}
# the flow algorithms: Markov clustering, with calls of its own (vg_cluster_mcl / vg_cluster_mcl_graph); always in the library
FLOW_ALGORITHMS = {'mcl': 6}
# every algorithm the library knows
LIBRARY_ALGORITHMS = {**CLUSTER_ALGORITHMS, **HIERARCHY_ALGORITHMS, **FLOW_ALGORITHMS}
# the algorithm of dereplicate (vg_dereplicate / vg_dereplicate_set): a genome is compared with representatives only, which is cd-hit
DEREP_ALGORITHMS = {'cd-hit': 1}
# genomes per batch of dereplicate ("Batch size")
DEREP_BATCH_GENOMES = 4096


class MclParams(C.Structure):
    _fields_ = [('inflation', C.c_double), ('prune', C.c_double), ('chaos_eps', C.c_double), ('max_row', C.c_int), ('max_iterations', C.c_int)]


class MclStats(C.Structure):
    _fields_ = [(name, C.c_int64) for name in ('iterations', 'converged', 'n_edges', 'nnz', 'max_row_seen', 'lds_rows', 'spill_rows')] + [('chaos', C.c_uint64)]


class DedupParams(C.Structure):
    _fields_ = [('gzip_level', C.c_int), ('num_threads', C.c_int), ('verbosity', C.c_int)]


class DedupStats(C.Structure):
    _fields_ = [('records', C.c_int64), ('unique', C.c_int64), ('removed', C.c_int64), ('reverse', C.c_int64),
                ('rounds', C.c_int64), ('collisions', C.c_int64)]


class DedupOptions(C.Structure):
    _fields_ = [('circular', C.c_int)]


class DedupContainedStats(C.Structure):
    _fields_ = [('passes', C.c_int64), ('positions', C.c_int64), ('hits', C.c_int64), ('candidates', C.c_int64),
                ('verified', C.c_int64), ('slices', C.c_int64)]


class DedupRepeatStats(C.Structure):
    _fields_ = [('with_repeat', C.c_int64), ('repeat_symbols', C.c_int64), ('candidates', C.c_int64), ('equal', C.c_int64),
                ('batches', C.c_int64)]


# The modes of deduplicate, keyed by (circular, contained, terminal repeat given): the C entry for files and the one for sequences;
# `extra`: the arguments that these two take beside the ones every mode has, from the terminal repeat; `n_arrays`: the int64 arrays
# the sequence entry fills beside representative and strand (the offsets, the repeats); `more_stats`: its second stats struct.
DedupMode = collections.namedtuple('DedupMode', 'files seqs extra n_arrays more_stats')
DEDUP_MODES = {
    (False, False, False): DedupMode('vg_deduplicate', 'vg_dedup_seqs', lambda tr: [], 0, None),
    (True, False, False): DedupMode('vg_deduplicate_ex', 'vg_dedup_seqs_ex', lambda tr: [C.byref(DedupOptions(circular=1))], 1, None),
    (True, False, True): DedupMode('vg_deduplicate_circular_tr', 'vg_dedup_seqs_circular_tr', lambda tr: [int(tr)], 2, DedupRepeatStats),
    (False, True, False): DedupMode('vg_deduplicate_contained', 'vg_dedup_seqs_contained', lambda tr: [], 1, DedupContainedStats),
}


def dedup_mode(circular, contained, repeat_given, needs='circular'):
    """The mode of deduplicate for these options, and its argument check; `needs`: how the caller spells the circular option."""
    if circular and contained:
        raise ValueError('circular and contained exclude each other')
    if repeat_given and not circular:
        raise ValueError(f'terminal_repeat needs {needs}')
    return DEDUP_MODES[bool(circular), bool(contained), bool(repeat_given)]


class KmerGeometry(C.Structure):
    _fields_ = [('accepted', C.c_int), ('P', C.c_int64), ('n_passes', C.c_int),
                ('levels', C.c_int), ('total_bits', C.c_int), ('B1', C.c_int), ('B2', C.c_int),
                ('st_tiles', C.c_int), ('n_st', C.c_int64), ('u_st', C.c_int), ('g_st', C.c_int),
                ('tile32k', C.c_int), ('narrow', C.c_int), ('short_rec', C.c_int)]


class KernelTime(C.Structure):
    _fields_ = [('name', C.c_char * 48), ('total_ms', C.c_double), ('launches', C.c_int64),
                ('bytes', C.c_double)]


ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int)

# every symbol include/vclust_gpu.h declares: (restype, argtypes)
P = C.POINTER
SYMBOLS = {
    'vg_version': (C.c_char_p, []),
    'vg_last_error': (C.c_char_p, []),
    'vg_free': (None, [C.c_void_p]),
    'vg_device_count': (C.c_int, []),
    'vg_set_device': (C.c_int, [C.c_int]),
    'vg_release_device_memory': (None, []),
    'vg_copy': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int]),
    'vg_alloc_selftest': (C.c_int, [C.POINTER(C.c_int64), C.c_int, C.c_int]),
    'vg_genomes_load': (C.c_int, [P(C.c_char_p), C.c_int, C.c_int, C.c_int, P(C.c_void_p)]),
    'vg_genomes_load_db_new': (C.c_int, [P(C.c_char_p), C.c_int, P(C.c_char_p), C.c_int, C.c_int, C.c_int, P(C.c_void_p), P(C.c_int)]),
    'vg_genomes_from_codes': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, P(C.c_char_p), P(C.c_void_p)]),
    'vg_genomes_free': (None, [C.c_void_p]),
    'vg_genomes_count': (C.c_int, [C.c_void_p]),
    'vg_genomes_total_len': (C.c_int64, [C.c_void_p]),
    'vg_genomes_lengths': (C.c_int, [C.c_void_p, P(C.c_int64)]),
    'vg_genomes_name': (C.c_char_p, [C.c_void_p, C.c_int]),
    'vg_genomes_codes': (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    'vg_genomes_to_device': (C.c_int, [C.c_void_p]),
    'vg_genomes_subset': (C.c_int, [C.c_void_p, P(C.c_int32), C.c_int, P(C.c_void_p)]),
    'vg_genomes_extend': (C.c_int, [C.c_void_p, C.c_void_p, P(C.c_int32), C.c_int]),
    'vg_genomes_truncate': (C.c_int, [C.c_void_p, C.c_int]),
    'vg_genomes_reserve': (C.c_int, [C.c_void_p, C.c_int64, C.c_int64]),
    'vg_kmer_shared': (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int, C.c_uint32,
                                 P(C.c_int64), P(P(PairCount)), P(C.c_int64)]),
    'vg_kmer_shared_new': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_uint32, P(C.c_int64), P(P(PairCount)), P(C.c_int64)]),
    'vg_kmer_geometry': (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int, P(KmerGeometry)]),
    'vg_kmer_geometry_at': (C.c_int, [C.c_int64, C.c_int, P(KmerGeometry)]),
    'vg_kmer_level2_slots': (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_int, P(C.c_int)]),
    'vg_rowptr_inline_lo': (C.c_int, [C.c_int64, C.c_int64, P(C.c_uint32)]),
    'vg_kmer_set': (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_double, P(P(C.c_uint64)), P(C.c_int64)]),
    'vg_filter_pairs': (C.c_int, [C.c_int, C.c_int, C.c_double, C.POINTER(C.c_int64), C.c_int64, C.POINTER(PairCount), C.c_int64,
                                  C.POINTER(C.POINTER(PairCount)), C.POINTER(C.c_int64)]),
    'vg_write_fltr': (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_double, C.c_int,
                                P(C.c_int64), P(PairCount), C.c_int64, C.c_char_p]),
    'vg_prefilter': (C.c_int, [P(C.c_char_p), C.c_int, C.c_char_p, P(PrefilterParams)]),
    'vg_prefilter_new': (C.c_int, [P(C.c_char_p), C.c_int, P(C.c_char_p), C.c_int, C.c_char_p, P(PrefilterParams)]),
    'vg_set_process_ends_after_call': (None, [C.c_int]),
    'vg_set_lz_fit': (None, [P(LzFit)]),
    'vg_lz_align': (C.c_int, [C.c_void_p, P(Task), C.c_int64, P(LzParams), P(PairStat),
                              P(P(Region)), P(C.c_int64)]),
    'vg_align_order': (C.c_int, [C.c_void_p, P(C.c_int32)]),
    'vg_read_filter': (C.c_int, [C.c_void_p, C.c_char_p, C.c_double, P(P(PairCount)), P(C.c_int64)]),
    'vg_align_tasks': (C.c_int, [C.c_void_p, P(PairCount), C.c_int64, P(P(Task)), P(C.c_int64)]),
    'vg_lz_prepare': (C.c_int, [C.c_void_p, P(PairCount), C.c_int64, P(LzParams)]),
    'vg_lz_index_dump': (C.c_int, [C.c_void_p, C.c_int, P(LzParams), P(P(C.c_uint32)), P(P(C.c_uint32)), P(C.c_int64),
                                   P(C.c_int), P(C.c_int), P(C.c_int)]),
    'vg_set_index_budget': (None, [C.c_int64]),
    'vg_set_subshards': (None, [C.c_int]),
    'vg_set_range_scan': (None, [C.c_int]),
    'vg_set_new_path': (None, [C.c_int]),
    'vg_set_placement_trials': (None, [C.c_int]),
    'vg_write_ani': (C.c_int, [C.c_void_p, P(Task), P(PairStat), C.c_int64, P(Region), C.c_int64,
                               C.c_char_p, P(AlignParams)]),
    'vg_align': (C.c_int, [P(C.c_char_p), C.c_int, C.c_char_p, P(AlignParams)]),
    'vg_align_new': (C.c_int, [P(C.c_char_p), C.c_int, P(C.c_char_p), C.c_int, C.c_char_p, P(AlignParams)]),
    'vg_comm_create': (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_void_p, P(C.c_void_p)]),
    'vg_rccl_unique_id': (C.c_int, [C.c_void_p, C.c_int64]),
    'vg_comm_rccl_create': (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_int64, P(C.c_void_p)]),
    'vg_comm_free': (None, [C.c_void_p]),
    'vg_comm_kind': (C.c_int, [C.c_void_p]),
    'vg_comm_rccl_ranks': (C.c_int, [C.c_void_p]),
    'vg_comm_rank': (C.c_int, [C.c_void_p]),
    'vg_comm_world': (C.c_int, [C.c_void_p]),
    'vg_comm_selftest': (C.c_int, [C.c_void_p, C.c_int64]),
    'vg_kmer_shared_sharded': (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_uint32, C.c_void_p, P(C.c_int64), P(P(PairCount)), P(C.c_int64)]),
    'vg_align_owner': (C.c_int, [P(Task), C.c_int64, C.c_int, C.c_int, P(C.c_int32)]),
    'vg_align_pairs_share': (C.c_int, [C.c_void_p, P(PairCount), C.c_int64, C.c_int, C.c_int, P(P(Task)), P(C.c_int64)]),
    'vg_lz_align_pairs_sharded': (C.c_int, [C.c_void_p, P(PairCount), C.c_int64, P(LzParams), C.c_void_p, P(P(Task)), P(C.c_int64), P(P(PairStat))]),
    'vg_lz_align_sharded': (C.c_int, [C.c_void_p, P(Task), C.c_int64, P(LzParams), C.c_void_p, P(PairStat), P(P(Region)), P(C.c_int64)]),
    'vg_prefilter_sharded': (C.c_int, [P(C.c_char_p), C.c_int, C.c_char_p, P(PrefilterParams), C.c_void_p]),
    'vg_align_sharded': (C.c_int, [P(C.c_char_p), C.c_int, C.c_char_p, P(AlignParams), C.c_void_p]),
    'vg_cluster': (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, P(ClusterParams)]),
    'vg_cluster_graph': (C.c_int, [C.c_int64, P(C.c_uint32), P(C.c_uint32), P(C.c_double), C.c_int64, C.c_int,
                                   P(C.c_int32), P(C.c_int32), P(ClusterStats)]),
    'vg_cluster_update_graph': (C.c_int, [C.c_int64, P(C.c_uint32), P(C.c_uint32), P(C.c_double), C.c_int64, C.c_int, P(C.c_int32),
                                          P(C.c_int32), P(C.c_int32), P(ClusterUpdateStats)]),
    'vg_cluster_update': (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, P(ClusterParams), P(ClusterUpdateStats)]),
    'vg_cluster_stats_graph': (C.c_int, [C.c_int64, P(C.c_uint32), P(C.c_uint32), P(C.c_double), C.c_int64, P(C.c_int32), C.c_int64,
                                         P(ClusterStat), P(C.c_uint64), P(C.c_uint64), P(C.c_int32)]),
    'vg_cluster_stats_file': (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, P(ClusterParams), C.c_char_p]),
    'vg_cluster_linkage_graph': (C.c_int, [C.c_int64, P(C.c_uint32), P(C.c_uint32), P(C.c_double), C.c_int64, P(C.c_int32), P(C.c_int32),
                                           P(C.c_double), P(C.c_int64), P(C.c_int64), P(C.c_int64), P(C.c_int64), P(LinkageStats)]),
    'vg_cluster_levels_graph': (C.c_int, [C.c_int64, P(C.c_uint32), P(C.c_uint32), P(C.c_double), C.c_int64, P(C.c_double), C.c_int,
                                          P(C.c_int32), P(C.c_int32), P(LinkageStats)]),
    'vg_cluster_complete_linkage_graph': (C.c_int, [C.c_int64, P(C.c_uint32), P(C.c_uint32), P(C.c_double), C.c_int64, P(C.c_int32), P(C.c_int32),
                                                    P(C.c_double), P(C.c_int64), P(C.c_int64), P(C.c_int64), P(C.c_int64), P(LinkageStats)]),
    'vg_cluster_complete_levels_graph': (C.c_int, [C.c_int64, P(C.c_uint32), P(C.c_uint32), P(C.c_double), C.c_int64, P(C.c_double), C.c_int,
                                                   P(C.c_int32), P(C.c_int32), P(LinkageStats)]),
    'vg_cluster_average_linkage_graph': (C.c_int, [C.c_int64, P(C.c_uint32), P(C.c_uint32), P(C.c_double), C.c_int64, C.c_double, P(C.c_int32),
                                                   P(C.c_int32), P(C.c_double), P(C.c_uint64), P(C.c_uint64), P(C.c_int64), P(C.c_int64),
                                                   P(C.c_int64), P(C.c_int64), P(LinkageStats)]),
    'vg_cluster_average_levels_graph': (C.c_int, [C.c_int64, P(C.c_uint32), P(C.c_uint32), P(C.c_double), C.c_int64, C.c_double, P(C.c_double),
                                                  C.c_int, P(C.c_int32), P(C.c_int32), P(LinkageStats)]),
    'vg_cluster_average_similarity': (C.c_double, [C.c_uint64, C.c_uint64]),
    'vg_cluster_average_order_selftest': (C.c_int, [P(C.c_uint64), P(C.c_uint32), P(C.c_uint32), P(C.c_uint32), P(C.c_uint32), C.c_int64,
                                                    C.c_int, P(C.c_int8)]),
    'vg_cluster_linkage': (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, P(ClusterParams), C.c_char_p, P(C.c_double), C.c_int]),
    'vg_cluster_mcl_graph': (C.c_int, [C.c_int64, P(C.c_uint32), P(C.c_uint32), P(C.c_double), C.c_int64, P(MclParams), P(C.c_int32), P(C.c_int32),
                                       P(P(C.c_int64)), P(P(C.c_int32)), P(P(C.c_uint32)), P(MclStats)]),
    'vg_cluster_mcl': (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, P(ClusterParams), P(MclParams), P(MclStats)]),
    'vg_cluster_mcl_set_table_slots': (None, [C.c_int]),
    'vg_cover_rows': (C.c_int, [C.c_int64, P(C.c_int64), P(C.c_int32), C.c_int64, P(C.c_uint32), P(C.c_uint32), P(C.c_int32), P(C.c_int32), C.c_int64,
                                P(CoverStat), P(P(CoverSegment)), P(C.c_int64), P(CoverRunStats)]),
    'vg_cover_file': (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int]),
    'vg_paint_rows': (C.c_int, [C.c_int64, P(C.c_int64), P(C.c_int32), C.c_int64, P(C.c_uint32), P(C.c_uint32), P(C.c_int32), P(C.c_int32), P(C.c_int32),
                                C.c_int64, P(PaintStat), P(P(PaintSegment)), P(C.c_int64), P(P(PaintDonor)), P(C.c_int64), P(PaintRunStats)]),
    'vg_paint_file': (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_int]),
    'vg_dereplicate_set': (C.c_int, [C.c_void_p, P(DerepParams), P(C.c_int32), P(C.c_int32), P(P(Task)), P(P(PairStat)), P(C.c_int64),
                                     P(DerepStats)]),
    'vg_dereplicate': (C.c_int, [P(C.c_char_p), C.c_int, C.c_char_p, P(DerepFileParams)]),
    'vg_dereplicate_update_set': (C.c_int, [C.c_void_p, C.c_int, P(DerepParams), P(C.c_int32), P(C.c_int32), P(C.c_int32), P(P(Task)), P(P(PairStat)),
                                            P(C.c_int64), P(DerepStats), P(DerepUpdateStats)]),
    'vg_dereplicate_update': (C.c_int, [P(C.c_char_p), C.c_int, P(C.c_char_p), C.c_int, C.c_char_p, C.c_int, C.c_char_p, P(DerepFileParams),
                                        P(DerepUpdateStats)]),
    'vg_deduplicate': (C.c_int, [P(C.c_char_p), C.c_int, P(C.c_char_p), C.c_char_p, C.c_char_p, P(DedupParams)]),
    'vg_dedup_seqs': (C.c_int, [C.c_char_p, P(C.c_int64), C.c_int64, P(C.c_int32), P(C.c_int8), P(DedupStats)]),
    'vg_deduplicate_ex': (C.c_int, [P(C.c_char_p), C.c_int, P(C.c_char_p), C.c_char_p, C.c_char_p, P(DedupParams), P(DedupOptions)]),
    'vg_dedup_seqs_ex': (C.c_int, [C.c_char_p, P(C.c_int64), C.c_int64, P(DedupOptions), P(C.c_int32), P(C.c_int8), P(C.c_int64),
                                   P(DedupStats)]),
    'vg_dedup_set_hash_bits': (None, [C.c_int]),
    'vg_dedup_terminal_repeats': (C.c_int, [C.c_char_p, P(C.c_int64), C.c_int64, C.c_int64, P(C.c_int64)]),
    'vg_dedup_seqs_circular_tr': (C.c_int, [C.c_char_p, P(C.c_int64), C.c_int64, C.c_int64, P(C.c_int32), P(C.c_int8), P(C.c_int64),
                                            P(C.c_int64), P(DedupStats), P(DedupRepeatStats)]),
    'vg_deduplicate_circular_tr': (C.c_int, [P(C.c_char_p), C.c_int, P(C.c_char_p), C.c_char_p, C.c_char_p, P(DedupParams), C.c_int64]),
    'vg_deduplicate_contained': (C.c_int, [P(C.c_char_p), C.c_int, P(C.c_char_p), C.c_char_p, C.c_char_p, P(DedupParams)]),
    'vg_dedup_seqs_contained': (C.c_int, [C.c_char_p, P(C.c_int64), C.c_int64, P(C.c_int32), P(C.c_int8), P(C.c_int64), P(DedupStats),
                                          P(DedupContainedStats)]),
    'vg_dedup_set_anchor_symbols': (None, [C.c_int]),
    'vg_dedup_set_index_positions': (None, [C.c_int64]),
    'vg_synth_plan': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_double, C.c_double, C.c_int,
                                C.c_int, P(C.c_void_p), P(C.c_void_p), P(C.c_int64)]),
    'vg_profile_enable': (None, [C.c_int]),
    'vg_profile_reset': (None, []),
    'vg_profile_get': (C.c_int, [P(KernelTime), C.c_int]),
}

_lib = None


def load():
    """Return the loaded library, binding all prototypes on first use."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ImportError(
            f'{LIB_PATH} is missing: the HIP extension is the product and has no fallback. '
            'Build it with `python -m vclust_amd.build` (needs hipcc).')
    lib = C.CDLL(str(LIB_PATH))
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)       # AttributeError if the .so does not export the symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise VclustGpuError(rc, load().vg_last_error().decode('utf-8', 'replace'))


# ---------------------------------------------------------------- marshalling (numpy-free: an array is anything with .ctypes)
def ptr(arr, ctype=None):
    """A pointer to the memory of an array: to `ctype` elements, or void*."""
    return arr.ctypes.data_as(C.POINTER(ctype) if ctype is not None else C.c_void_p)


def path(p):
    """A path as the bytes of a char* argument; None stays None (NULL)."""
    return None if p is None else os.fsencode(str(p))


def path_array(paths):
    return (C.c_char_p * len(paths))(*[path(p) for p in paths])


def string_array(strings):
    return (C.c_char_p * len(strings))(*[str(s).encode() for s in strings])


def as_dict(*structs):
    """The fields of the structs, in order, as one dict."""
    return {name: getattr(st, name) for st in structs for name, _ in st._fields_}


def hip_copy(dst, src, nbytes, to_host):
    check(load().vg_copy(C.c_void_p(int(dst) if not isinstance(dst, C.c_void_p) else dst.value), C.c_void_p(int(src) if not isinstance(src, C.c_void_p) else src.value),
                         int(nbytes), int(bool(to_host))))
