"""The whole-stage calls of the drop-in CLI (vg_prefilter, vg_align: FASTA on disk -> fltr.txt / ani.tsv on disk; vg_cluster:
ani.tsv + ids file -> clusters.tsv, vg_cluster_stats_file: the per-cluster report of a clusters.tsv; vg_cover_file: the alignment table of align -> the coverage map; vg_paint_file: the same table -> the closest partner at every position; vg_deduplicate: FASTA files -> distinct records + duplicates list) as thin ctypes wrappers WITHOUT numpy: a `vclust.py prefilter|align|cluster|deduplicate` process is
one of these calls, and importing numpy costs it 60-180 ms of its ~1 s.  vclust_amd.api re-exports them beside the
array-level API."""
import ctypes as C
import os

from . import _lib
from ._lib import (ALIGN_OUTFMT, DEFAULT_LZ, DEREP_ALGORITHMS, DEREP_BATCH_GENOMES, FLOW_ALGORITHMS, HIERARCHY_ALGORITHMS, LIBRARY_ALGORITHMS,  # noqa: F401
                   UPDATE_ALGORITHMS, AlignParams, ClusterParams, ClusterUpdateStats, DedupParams, DerepFileParams, DerepParams,
                   DerepStats, DerepUpdateStats, MclParams, MclStats, PrefilterParams, as_dict, check, lz_params, path, path_array, string_array)


def dist_env():
    """(rank, world, local_rank) of a torchrun launch, (0, 1, 0) otherwise."""
    return int(os.environ.get('RANK', '0')), int(os.environ.get('WORLD_SIZE', '1')), int(os.environ.get('LOCAL_RANK', '0'))


def _check_prior(prior_path, prior_repr):
    if prior_path is None and prior_repr:
        raise ValueError('prior_repr needs prior_path')


def prefilter(paths, out_path, is_multifasta, k=25, min_kmers=20, min_ident=0.7, batch_size=0,
              kmers_fraction=1.0, max_seqs=0, num_threads=1, verbosity=0, db_paths=None):
    """fltr.txt of the genomes in `paths` (vg_prefilter).  db_paths: a database the genomes of `paths` are new to -- the set is
    the database's genomes followed by them, and only the rows of the new genomes are filled (vg_prefilter_new)."""
    lib = _lib.load()
    prm = PrefilterParams(k, min_kmers, min_ident, batch_size, kmers_fraction, max_seqs, num_threads,
                          verbosity, int(bool(is_multifasta)))
    if db_paths is not None:
        check(lib.vg_prefilter_new(path_array(db_paths), len(db_paths), path_array(paths), len(paths), path(out_path), C.byref(prm)))
        return
    check(lib.vg_prefilter(path_array(paths), len(paths), path(out_path), C.byref(prm)))


def align_params(columns, filter_path=None, filter_threshold=0.0, out_aln=None, lz=None, out_filters=None, num_threads=1,
                 verbosity=0, is_multifasta=True):
    """vg_align_params for the given options (the struct keeps its strings alive through attributes)."""
    cols = string_array(columns)
    p = AlignParams()
    p.lz = lz_params(lz)
    for name, val in (out_filters or {}).items():
        setattr(p, f'out_{name}', float(val))
    p.filter_path = path(filter_path or None)
    p.filter_threshold = float(filter_threshold)
    p.out_aln_path = path(out_aln or None)
    p.out_columns = cols
    p.n_out_columns = len(columns)
    p.num_threads = num_threads
    p.verbosity = verbosity
    p.is_multifasta = int(bool(is_multifasta))
    p._keep = cols
    return p


def align(paths, out_path, is_multifasta, columns, filter_path=None, filter_threshold=0.0, out_aln=None,
          lz=None, out_filters=None, num_threads=1, verbosity=0, db_paths=None):
    """ani.tsv of the genomes in `paths` (vg_align).  db_paths: as in prefilter; only pairs that contain a genome of `paths` are
    aligned -- the filter's, or all of them without a filter (vg_align_new)."""
    lib = _lib.load()
    p = align_params(columns, filter_path, filter_threshold, out_aln, lz, out_filters, num_threads, verbosity, is_multifasta)
    if db_paths is not None:
        check(lib.vg_align_new(path_array(db_paths), len(db_paths), path_array(paths), len(paths), path(out_path), C.byref(p)))
        return
    check(lib.vg_align(path_array(paths), len(paths), path(out_path), C.byref(p)))


CLUSTER_FILTERS = ('tani', 'gani', 'ani', 'qcov', 'rcov', 'len_ratio')
# the keywords of cluster() that belong to algorithm='mcl', with the library's defaults
MCL_DEFAULTS = dict(mcl_inflation=2.0, mcl_prune=1e-4, mcl_max_row=128, mcl_chaos_eps=1e-3, mcl_iterations=100)


def _cluster_params(algorithm_code, metric, num_alns, representatives, num_threads, verbosity, mins):
    """vg_cluster_params of cluster() and cluster_stats(); mins: the minimum per filter of CLUSTER_FILTERS."""
    unknown = set(mins) - set(CLUSTER_FILTERS)
    if unknown:
        raise TypeError(f'unknown filter(s): {sorted(unknown)}')
    p = ClusterParams(algorithm=algorithm_code, metric=metric.encode(), max_num_alns=int(num_alns), representatives=int(bool(representatives)),
                      num_threads=int(num_threads), verbosity=int(verbosity))
    for name, val in mins.items():
        setattr(p, f'min_{name}', float(val))
    return p


def cluster(ani_path, ids_path, out_path, algorithm='single', metric='tani', num_alns=0, representatives=False,
            num_threads=0, verbosity=0, out_linkage=None, levels=None, prior_path=None, prior_repr=False, **mins):
    """clusters.tsv from ani.tsv + its ids file (vg_cluster).  mins: tani=, gani=, ani=, qcov=, rcov=, len_ratio= (0 = off);
    num_alns: max. number of local alignments of a passing row (0 = off).  out_linkage: also the merge table
    -> that file; levels: one more column per level, the cut of the same forest there (vg_cluster_linkage; both need
    algorithm='single', 'complete' or 'average' -- the merge table and the cuts of that hierarchy -- and no level below the metric's
    minimum).  algorithm='complete' or 'average' without either is the cut of that hierarchy at the floor (vg_cluster).  'average'
    (UPGMA in exact arithmetic; a pair without a row counts as 0) stops at the metric's minimum, and its cut at a level is not
    a run at that minimum: the rows between the two still count in the averages.  prior_path: a clusters.tsv of an earlier run
    whose clusters are taken as given and to which the other objects of the ids file are added (vg_cluster_update; algorithm
    'single', 'cd-hit' or 'uclust', no out_linkage and no levels); prior_repr: its second column holds representative ids.  That
    call returns the update's counts as a dict.  algorithm='mcl': Markov clustering (vg_cluster_mcl; DESIGN.md section 9, "Markov
    clustering"), deterministic, with the keywords mcl_inflation (a multiple of 0.5 in [1.5, 6]), mcl_prune, mcl_max_row,
    mcl_chaos_eps and mcl_iterations; it excludes prior_path, out_linkage and levels and returns its stats as a dict (iterations,
    converged, chaos, ...).  Every other call returns None."""
    mcl = {k: mins.pop(k) for k in list(mins) if k in MCL_DEFAULTS}
    # (an unknown filter is the first error; an unknown algorithm is refused below, before p is used)
    p = _cluster_params(LIBRARY_ALGORITHMS.get(algorithm, 0), metric, num_alns, representatives, num_threads, verbosity, mins)
    if mcl and algorithm not in FLOW_ALGORITHMS:
        raise ValueError(f'{", ".join(sorted(mcl))}: only with algorithm=\'mcl\'')
    _check_prior(prior_path, prior_repr)
    hierarchy = out_linkage is not None or levels is not None
    if prior_path is not None:
        if hierarchy:
            raise ValueError('prior_path excludes out_linkage and levels')
        if algorithm not in UPDATE_ALGORITHMS:
            raise ValueError(f'algorithm {algorithm!r} cannot update a prior clustering (choices: {", ".join(UPDATE_ALGORITHMS)})')
    if algorithm not in LIBRARY_ALGORITHMS:
        raise ValueError(f'algorithm {algorithm!r} is not computed by the library (choices: {", ".join(LIBRARY_ALGORITHMS)})')
    paths = (path(ani_path), path(ids_path), path(out_path))
    if prior_path is not None:
        st = ClusterUpdateStats()
        check(_lib.load().vg_cluster_update(paths[0], paths[1], path(prior_path), int(bool(prior_repr)), paths[2], C.byref(p), C.byref(st)))
        return as_dict(st)
    if algorithm in FLOW_ALGORITHMS and not hierarchy:
        m = {**MCL_DEFAULTS, **mcl}
        prm = MclParams(float(m['mcl_inflation']), float(m['mcl_prune']), float(m['mcl_chaos_eps']), int(m['mcl_max_row']), int(m['mcl_iterations']))
        st = MclStats()
        check(_lib.load().vg_cluster_mcl(*paths, C.byref(p), C.byref(prm), C.byref(st)))
        return as_dict(st)
    if not hierarchy:
        check(_lib.load().vg_cluster(*paths, C.byref(p)))
        return
    if algorithm not in HIERARCHY_ALGORITHMS:
        raise ValueError('out_linkage and levels need algorithm=\'single\', \'complete\' or \'average\'')
    lv = [float(x) for x in (levels or ())]
    check(_lib.load().vg_cluster_linkage(*paths, C.byref(p), path(out_linkage), (C.c_double * len(lv))(*lv) if lv else None, len(lv)))


def cluster_stats(ani_path, ids_path, clusters_path, out_path, clusters_repr=False, metric='tani', num_alns=0, num_threads=0,
                  verbosity=0, **mins):
    """The cohesion / separation report of a clusters.tsv (vg_cluster_stats_file; DESIGN.md section 9, "Cluster report") -> out_path:
    one block per label column, one line per cluster (members, pairs with a row, weakest and mean similarity inside, the nearest
    other cluster, members closer to another cluster than to their own).  The rows are those of ani.tsv that pass the filters of
    cluster() (metric, mins, num_alns: give the ones the clustering was made with); clusters_path may be any clustering of the
    ids file, this library's or not; clusters_repr: its label columns hold representative ids."""
    p = _cluster_params(0, metric, num_alns, False, num_threads, verbosity, mins)
    check(_lib.load().vg_cluster_stats_file(path(ani_path), path(ids_path), path(clusters_path), int(bool(clusters_repr)), C.byref(p),
                                            path(out_path)))


def cover(aln_path, ids_path, out_path, clusters_path=None, clusters_repr=False, column=None, segments_path=None, num_threads=0,
          verbosity=0):
    """The coverage map of an alignment table (vg_cover_file): aln_path is the file `align --out-aln` writes,
    ids_path its ids file.  -> out_path: one line per genome (partners, covered positions, core, depths); segments_path: also the
    depth profile, one line per maximal run of constant depth.  clusters_path: a clusters.tsv whose label column `column` (default:
    the first) gives the groups that split the depth into `in` and `out`; clusters_repr: its label columns hold representative
    ids.  Without it all genomes are one group."""
    if clusters_path is None and (clusters_repr or column is not None):
        raise ValueError('clusters_repr and column describe the file of clusters_path: they need clusters_path')
    check(_lib.load().vg_cover_file(path(aln_path), path(ids_path), path(clusters_path), int(bool(clusters_repr)),
                                    None if column is None else str(column).encode(), path(out_path), path(segments_path), int(num_threads),
                                    int(verbosity)))


def paint(aln_path, ids_path, out_path, clusters_path=None, clusters_repr=False, column=None, segments_path=None, donors_path=None,
          num_threads=0, verbosity=0):
    """The mosaic painting of an alignment table (vg_paint_file): aln_path is the file `align --out-aln` writes,
    ids_path its ids file.  At every position of a genome the row of the highest identity that covers it wins.  -> out_path: one
    line per genome (painted positions, donors, the top partner, switches, segments); segments_path: also one line per maximal run
    of one winning row, with its partner and pident; donors_path: also one line per (genome, winning partner).  clusters_path,
    clusters_repr and column as in cover(): the groups that split the painted positions into `in` and `out`."""
    if clusters_path is None and (clusters_repr or column is not None):
        raise ValueError('clusters_repr and column describe the file of clusters_path: they need clusters_path')
    check(_lib.load().vg_paint_file(path(aln_path), path(ids_path), path(clusters_path), int(bool(clusters_repr)),
                                    None if column is None else str(column).encode(), path(out_path), path(segments_path), path(donors_path),
                                    int(num_threads), int(verbosity)))


def deduplicate(paths, out_path, dup_path, prefixes=None, gzip_level=0, num_threads=0, verbosity=0, circular=False, contained=False,
                terminal_repeat=0):
    """The distinct records of the FASTA files `paths` -> out_path, the removed ones -> dup_path (vg_deduplicate).
    prefixes: None or one string per path, put in front of every header of that file; gzip_level 0 = plain output.
    circular: rotations of a record and of its reverse complement are duplicates too, and dup_path gets an offset column
    (vg_deduplicate_ex).  contained: records that are substrings of a longer record or of its reverse complement are removed
    too, with the same offset column (vg_deduplicate_contained); it excludes circular.  terminal_repeat (with circular only):
    an exact repeat of a record's first symbols at its end, of at least that many symbols, is taken off before rotations are
    compared, and dup_path gets the two repeat columns (vg_deduplicate_circular_tr); 0 = off."""
    mode = _lib.dedup_mode(circular, contained, terminal_repeat)
    if prefixes is not None and len(prefixes) != len(paths):
        raise ValueError('one prefix per input file')
    prm = DedupParams(gzip_level=int(gzip_level), num_threads=int(num_threads), verbosity=int(verbosity))
    check(getattr(_lib.load(), mode.files)(path_array(paths), len(paths), string_array(prefixes) if prefixes is not None else None,
                                           path(out_path), path(dup_path), C.byref(prm), *mode.extra(terminal_repeat)))


def derep_params(batch_genomes=None, k=25, kmers_fraction=1.0, min_kmers=20, min_ident=0.7, lz=None, algorithm='cd-hit', metric='tani',
                 num_alns=0, mins=None):
    """vg_derep_params of dereplicate() and GenomeSet.dereplicate_set().  An algorithm the library does not know at all is refused
    here; one it knows but dereplicate cannot run (anything but cd-hit) is refused by the library, before any device use."""
    if algorithm not in LIBRARY_ALGORITHMS:
        raise ValueError(f'algorithm {algorithm!r} is not computed by the library (choices of dereplicate: {", ".join(DEREP_ALGORITHMS)})')
    p = DerepParams()
    p.k, p.kmers_fraction, p.min_kmers, p.min_ident = int(k), float(kmers_fraction), int(min_kmers), float(min_ident)
    p.lz = lz_params(lz)
    p.cluster = _cluster_params(LIBRARY_ALGORITHMS[algorithm], metric, num_alns, False, 0, 0, mins or {})
    p.batch_genomes = DEREP_BATCH_GENOMES if batch_genomes is None else int(batch_genomes)
    return p


def dereplicate(paths, out_path, is_multifasta, batch_genomes=None, k=25, kmers_fraction=1.0, min_kmers=20, min_ident=0.7, lz=None,
                algorithm='cd-hit', metric='tani', num_alns=0, representatives=False, out_table=None, columns=None, out_repr_fasta=None,
                num_threads=1, verbosity=0, db_paths=None, prior_path=None, prior_repr=False, **mins):
    """clusters.tsv of the genomes in `paths` by greedy clustering against representatives only (vg_dereplicate; DESIGN.md section
    13): the file that prefilter -> align with that filter -> cluster(algorithm='cd-hit') writes for the same options, for every
    batch_genomes.  out_table: also an ani.tsv of the rows that were computed (columns: default the standard format) and its
    .ids.tsv; out_repr_fasta: the records of the representatives, verbatim (one multi-FASTA input only).  db_paths and prior_path
    (both or neither): the genomes of `paths` are new to the database db_paths, whose clusters -- the clusters.tsv prior_path of
    an earlier run, prior_repr: with representative ids in its second column -- are kept as they are (vg_dereplicate_update): the
    file that prefilter, align and cluster(prior_path=...) write with db_paths, with only the prior representatives ever compared.
    -> the counts as a dict."""
    if (db_paths is None) != (prior_path is None):
        raise ValueError('db_paths and prior_path go together: the database is the genome set of the prior clustering')
    _check_prior(prior_path, prior_repr)
    st, ust = DerepStats(), DerepUpdateStats()
    p = DerepFileParams()
    p.derep = derep_params(batch_genomes, k, kmers_fraction, min_kmers, min_ident, lz, algorithm, metric, num_alns, mins)
    p.representatives = int(bool(representatives))
    columns = list(columns or ALIGN_OUTFMT['standard'])
    cols = string_array(columns)
    p.out_table_path = path(out_table)
    p.out_columns, p.n_out_columns = cols, len(columns)
    p.out_repr_fasta_path = path(out_repr_fasta)
    p.num_threads, p.verbosity, p.is_multifasta = int(num_threads), int(verbosity), int(bool(is_multifasta))
    p.stats = C.pointer(st)
    if db_paths is None:
        check(_lib.load().vg_dereplicate(path_array(paths), len(paths), path(out_path), C.byref(p)))
        return as_dict(st)
    check(_lib.load().vg_dereplicate_update(path_array(db_paths), len(db_paths), path_array(paths), len(paths), path(prior_path),
                                            int(bool(prior_repr)), path(out_path), C.byref(p), C.byref(ust)))
    return as_dict(st, ust)
