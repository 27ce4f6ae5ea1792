"""Vclust-compatible command line (drop-in for the reference's vclust.py, v1.3.1 surface).

`prefilter` and `align` keep the reference's options, defaults, messages, exit codes and
output files (vclust.py:178-421, 1380-1521) but call libvclust_gpu.so (HIP, MI355X) through
ctypes instead of running bin/kmer-db and bin/lz-ani as subprocesses.  `cluster` passes its
arguments on to bin/clusty where that binary exists, as the reference does; without it, the
single, cd-hit, uclust and set-cover algorithms run on the GPU (vg_cluster); `--out-linkage` and
`--levels` (the merge table of single, complete or average linkage and its cuts) always run on the GPU, and so do `--algorithm average`,
`--algorithm mcl` (Markov clustering in exact integer arithmetic: vg_cluster_mcl)
and `--prior` (new genomes added to the clusters of an earlier clusters.tsv: vg_cluster_update); `--out-stats` is a second call
after clusters.tsv is written, whoever wrote it (the per-cluster report: vg_cluster_stats_file).  `deduplicate` does
the same with bin/mfasta-tool: the pass-through where that binary exists, the GPU (vg_deduplicate)
without it; `--circular` (with `--terminal-repeat <int>`: assembler overlaps taken off first) and
`--contained` always run on the GPU.  `dereplicate` (this repository's command: prefilter, align and cd-hit clustering in one
process, every genome compared with the representatives only; vg_dereplicate; with `--db` and `--prior` new genomes added to the
clusters of an earlier run, vg_dereplicate_update) always runs on the GPU.  `info` reports the library and the optional CPU tools.

Multi-GPU: start one process per GPU, e.g.
    python -m torch.distributed.run --nproc-per-node 8 vclust.py align -i x.fna -o ani.tsv ...
Each rank computes its share of the integer work; rows are gathered on rank 0 over RCCL.
"""
import argparse
import logging
import multiprocessing
import os
import pathlib
import subprocess
import sys

from . import stages
from ._lib import ALIGN_FIELDS, ALIGN_OUTFMT, CLUSTER_ALGORITHMS, DEFAULT_LZ, HIERARCHY_ALGORITHMS, UPDATE_ALGORITHMS  # noqa: F401
from .stages import CLUSTER_FILTERS, dist_env

__version__ = '1.3.1'

DEFAULT_THREAD_COUNT = min(multiprocessing.cpu_count(), 64)

SCRIPT_DIR = pathlib.Path(__file__).resolve().parent.parent
BIN_DIR = SCRIPT_DIR / 'bin'
BIN_CLUSTY = BIN_DIR / 'clusty'
BIN_MFASTA = BIN_DIR / 'mfasta-tool'

# ------------------------------------------------------------------ argument parsing
class _HelpFormatter(argparse.RawDescriptionHelpFormatter):
    def _format_action_invocation(self, action):
        if not action.option_strings or action.nargs == 0:
            return super()._format_action_invocation(action)
        metavar = self._format_args(action, self._get_default_metavar_for_optional(action))
        return ', '.join(action.option_strings) + ' ' + metavar

    def _split_lines(self, text, width):
        out = []
        for part in text.splitlines():
            out.extend(argparse.HelpFormatter._split_lines(self, part, width))
        return out


def _existing_path(value):
    path = pathlib.Path(value)
    if not path.exists():
        raise argparse.ArgumentTypeError(f'input does not exist: {value}')
    return path


def _unit_float(value):
    f = float(value)
    if f < 0 or f > 1:
        raise argparse.ArgumentTypeError('must be between 0 and 1')
    return f


# ------------------------------------------------------------------ option groups: each declared once, for every subcommand that takes it
LZ_HELP = dict(mal='Min. anchor length', msl='Min. seed length', mrd='Max. dist. between approx. matches in reference',
               mqd='Max. dist. between approx. matches in query', reg='Min. considered region length', aw='Approx. window length',
               am='Max. no. of mismatches in approx. window', ar='Min. length of run ending approx. extension')


def lz_options(p):
    for name, default in DEFAULT_LZ.items():
        p.add_argument(f'--{name}', metavar='<int>', type=int, default=default, help=f'{LZ_HELP[name]} [%(default)s]')


def prefilter_options(p, k_for, own=False):
    """-k, --min-kmers, --min-ident and --kmers-fraction; own: with the two options that only `prefilter` has, in its order."""
    p.add_argument('-k', '--k', metavar='<int>', type=int, default=25, choices=range(15, 31), help=f'Size of k-mer for {k_for} [%(default)s]')
    p.add_argument('--min-kmers', metavar='<int>', type=int, default=20,
                   help='Minimum number of shared k-mers between two genomes [%(default)s]')
    p.add_argument('--min-ident', metavar='<float>', type=_unit_float, default=0.7,
                   help='Minimum sequence identity (0-1) between two genomes, relative to the shorter one [%(default)s]')
    if own:
        p.add_argument('--batch-size', metavar='<int>', type=int, default=0,
                       help='Process a multifasta file in batches of <int> sequences (accepted for '
                            'compatibility; the GPU path produces identical results) [%(default)s]')
    p.add_argument('--kmers-fraction', metavar='<float>', type=_unit_float, default=1.0,
                   help='Fraction of k-mers to analyze in each genome (0-1) [%(default)s]')
    if own:
        p.add_argument('--max-seqs', metavar='<int>', type=int, default=0,
                       help='Maximum number of sequences allowed to pass the prefilter per query; 0 = all [%(default)s]')


def cluster_filter_options(p, **algorithm):
    """-r, --algorithm (default, choices and help are the subcommand's), --metric, the six minimums and --num_alns."""
    p.add_argument('-r', '--out-repr', action='store_true', dest='representatives',
                   help='Output a representative genome for each cluster [%(default)s]')
    p.add_argument('--algorithm', metavar='<str>', dest='algorithm', **algorithm)
    p.add_argument('--metric', metavar='<str>', dest='metric', choices=['tani', 'gani', 'ani'], default='tani',
                   help='Similarity metric for clustering [%(default)s]')
    for name in CLUSTER_FILTERS:
        p.add_argument(f'--{name}', metavar='<float>', dest=name, type=_unit_float, default=0, help=f'Min. {name} (0-1) [%(default)s]')
    p.add_argument('--num_alns', metavar='<int>', dest='num_alns', type=int, default=0,
                   help='Max. number of local alignments between two genomes; 0 = all [%(default)s]')


def prior_options(p, prior_help):
    p.add_argument('--prior', metavar='<file>', type=_existing_path, dest='prior_path', help=prior_help)
    p.add_argument('--prior-repr', action='store_true', dest='prior_repr',
                   help='The second column of --prior holds representative ids, as --out-repr writes them [%(default)s]')


def db_option(p):
    p.add_argument('--db', metavar='<file>', type=_existing_path, dest='db_path',
                   help='Database of genomes already processed (a FASTA file, or a directory of files, like -i): the genomes '
                        'of -i are new to it, the genome set is the database followed by them, and only pairs that contain a '
                        'new genome are computed (rows of an earlier run are matched by name: ids are those of the combined set)')


def lz_of(args):
    return {k: getattr(args, k) for k in DEFAULT_LZ}


def minimums_of(args):
    """The minimums that are set: as the reference, a filter is passed on only for a value > 0."""
    return {k: getattr(args, k) for k in CLUSTER_FILTERS if getattr(args, k) > 0}


# the groups as the 'Running:' line shows them
def _lz_text(args):
    return ' '.join(f'--{k} {v}' for k, v in lz_of(args).items())


def _prefilter_text(args):
    return f'-k {args.k} --min-kmers {args.min_kmers} --min-ident {args.min_ident} --kmers-fraction {args.kmers_fraction}'


def _filters_text(args):
    return (f' --metric {args.metric}' + ''.join(f' --{k} {v}' for k, v in minimums_of(args).items())
            + (f' --num_alns {args.num_alns}' if args.num_alns > 0 else '') + (' --out-repr' if args.representatives else ''))


def _prior_text(args):
    if getattr(args, 'prior_path', None) is None:
        return ''
    return f' --prior {args.prior_path}' + (' --prior-repr' if args.prior_repr else '')


def get_parser() -> argparse.ArgumentParser:
    fmt = lambda prog: _HelpFormatter(prog, max_help_position=32, width=100)  # noqa: E731

    def common(p, threads=True):
        if threads:
            p.add_argument('-t', '--threads', metavar='<int>', dest='num_threads', type=int,
                           default=DEFAULT_THREAD_COUNT, help='Number of threads [%(default)s]')
        p.add_argument('-v', metavar='<int>', dest='verbosity_level', type=int, choices=[0, 1, 2], default=1,
                       help='Verbosity level [%(default)s]:\n0: Errors only\n1: Info\n2: Debug')
        p.add_argument('-h', '--help', action='help', help='Show this help message and exit')

    def io_args(p, in_help):
        req = p.add_argument_group('required arguments')
        req.add_argument('-i', '--in', metavar='<file>', type=_existing_path, dest='input_path', help=in_help,
                         required=True)
        req.add_argument('-o', '--out', metavar='<file>', type=pathlib.Path, dest='output_path',
                         help='Output filename', required=True)
        return req

    parser = argparse.ArgumentParser(
        description=f'%(prog)s v{__version__}: calculate ANI and cluster virus (meta)genome sequences '
                    '(MI355X-native prefilter/align)',
        formatter_class=fmt, add_help=False)
    parser.add_argument('-v', '--version', action='version', version=f'v{__version__}',
                        help="Display the tool's version and exit")
    parser.add_argument('-h', '--help', action='help', help='Show this help message and exit')
    sub = parser.add_subparsers(dest='command')

    # deduplicate (bin/mfasta-tool if present, else vg_deduplicate)
    dd = sub.add_parser('deduplicate', help='Deduplicate and merge genome sequences from multiple FASTA files',
                        formatter_class=fmt, add_help=False)
    ddr = dd.add_argument_group('required arguments')
    ddr.add_argument('-i', '--in', metavar='<file>', type=_existing_path, dest='input_path', nargs='+',
                     help='Space-separated input FASTA files (gzipped or uncompressed)')
    ddr.add_argument('-o', '--out', metavar='<file>', type=pathlib.Path, dest='output_path', required=True,
                     help='Output FASTA file with unique, nonredundant sequences')
    dd.add_argument('--add-prefixes', metavar='<str>', nargs='*', default=False,
                    help='Add prefixes to sequence IDs [%(default)s]')
    dd.add_argument('--gzip-output', action='store_true', help='Compress the output FASTA file with gzip')
    dd.add_argument('--gzip-level', metavar='<int>', type=int, default=4, help='Compression level (1-9) [%(default)s]')
    dd.add_argument('--circular', action='store_true',
                    help='Circular genomes: rotations of a sequence and of its reverse complement are duplicates too')
    dd.add_argument('--terminal-repeat', metavar='<int>', type=int, default=None,
                    help='Min. length of an exact terminal repeat (the same bases at both ends of a record, as assemblers leave on '
                         'circular contigs) taken off before rotations are compared; needs --circular')
    dd.add_argument('--contained', action='store_true',
                    help='Fragments: a sequence that is a contiguous substring of a longer sequence or of its reverse complement is removed too')
    common(dd)

    # prefilter
    pf = sub.add_parser('prefilter', help='Prefilter genome pairs for alignment', formatter_class=fmt, add_help=False)
    io_args(pf, 'Input FASTA file or directory of files (gzipped or uncompressed)')
    db_option(pf)
    prefilter_options(pf, 'Kmer-db', own=True)
    common(pf)

    # align
    al = sub.add_parser('align', help='Align genome sequence pairs and calculate ANI measures',
                        formatter_class=fmt, add_help=False)
    io_args(al, 'Input FASTA file or directory of files (gzipped or uncompressed)')
    db_option(al)
    al.add_argument('--filter', metavar='<file>', type=_existing_path, dest='filter_path',
                    help='Path to filter file (output of prefilter)')
    al.add_argument('--filter-threshold', metavar='<float>', dest='filter_threshold', type=_unit_float, default=0,
                    help='Align genome pairs above the threshold (0-1) [%(default)s]')
    al.add_argument('--outfmt', metavar='<str>', choices=ALIGN_OUTFMT.keys(), dest='outfmt', default='standard',
                    help='Output format [%(default)s]\nchoices: ' + ','.join(ALIGN_OUTFMT.keys()))
    al.add_argument('--out-aln', metavar='<file>', type=pathlib.Path, dest='aln_path',
                    help='Write alignments to the tsv <file>')
    for name, label in (('ani', 'ANI'), ('tani', 'tANI'), ('gani', 'gANI'),
                        ('qcov', 'query coverage (aligned fraction)'), ('rcov', 'reference coverage (aligned fraction)')):
        al.add_argument(f'--out-{name}', dest=name, metavar='<float>', type=_unit_float, default=0,
                        help=f'Min. {label} to output (0-1) [%(default)s]')
    lz_options(al)
    common(al)

    # cluster (bin/clusty if present, else vg_cluster for single / cd-hit / uclust / set-cover)
    cl = sub.add_parser('cluster', help='Cluster genomes based on ANI thresholds', formatter_class=fmt, add_help=False)
    clr = io_args(cl, 'Input file with ANI metrics (tsv)')
    clr.add_argument('--ids', metavar='<file>', type=_existing_path, dest='ids_path', required=True,
                     help='Input file with sequence identifiers (tsv)')
    cluster_filter_options(
        cl, default='single', choices=['single', 'complete', 'average', 'uclust', 'cd-hit', 'set-cover', 'leiden', 'mcl'],
        help='Clustering algorithm [%(default)s]; average (UPGMA: a pair without a row counts as 0) always runs on the GPU '
             'and merges down to the threshold of --metric; mcl (Markov clustering: deterministic, separates dense groups '
             'joined by weak rows) always runs on the GPU too')
    cl.add_argument('--out-linkage', metavar='<file>', type=pathlib.Path, dest='linkage_path',
                    help='Write the merge table of --algorithm single, complete or average (the dendrogram: one line per merge) '
                         'to the tsv <file>')
    cl.add_argument('--levels', metavar='<float>', type=_unit_float, nargs='+', dest='levels',
                    help='Further thresholds of the metric (0-1, none below its minimum): one more column per level, the cut of '
                         'the same hierarchy (single, complete or average linkage) there; under average linkage the cut at a level '
                         'is not a run at that threshold: the rows between the two still count in the averages')
    prior_options(cl, 'clusters.tsv of an earlier run: its clusters are taken as given and the other genomes of --ids are added '
                      'to them (--algorithm single, cd-hit or uclust; always runs on the GPU).  Under cd-hit and uclust every '
                      'earlier cluster keeps its members and its representative; under single, earlier clusters may merge')
    cl.add_argument('--out-stats', metavar='<file>', type=pathlib.Path, dest='stats_path',
                    help='After the clustering, write a per-cluster report to the tsv <file> (always on the GPU, for every '
                         '--algorithm): members, pairs with a row in the input, weakest and mean similarity inside the cluster, '
                         'the nearest other cluster, and members that are closer to another cluster than to their own')
    cl.add_argument('--mcl-inflation', metavar='<float>', type=float, dest='mcl_inflation', default=2.0,
                    help='--algorithm mcl: the inflation exponent, a multiple of 0.5 in 1.5-6 (halves keep the integer arithmetic '
                         'exact: pow() is not correctly rounded on the GPU); higher gives smaller clusters [%(default)s]')
    cl.add_argument('--mcl-prune', metavar='<float>', type=float, dest='mcl_prune', default=1e-4,
                    help='--algorithm mcl: drop flow below this share of a row (0-0.1) [%(default)s]')
    cl.add_argument('--mcl-max-row', metavar='<int>', type=int, dest='mcl_max_row', default=128,
                    help='--algorithm mcl: keep at most this many entries per row (2-4096) [%(default)s]')
    cl.add_argument('--mcl-iterations', metavar='<int>', type=int, dest='mcl_iterations', default=100,
                    help='--algorithm mcl: stop after this many iterations (1-1000) even if the flow still moves [%(default)s]')
    cl.add_argument('--leiden-resolution',metavar='<float>', type=_unit_float, default=0.7)
    cl.add_argument('--leiden-beta', metavar='<float>', type=_unit_float, default=0.01)
    cl.add_argument('--leiden-iterations', metavar='<int>', type=int, default=2)
    common(cl, threads=False)

    # dereplicate (always vg_dereplicate: this repository's command)
    dr = sub.add_parser('dereplicate', help='Cluster genomes into representatives (greedy, cd-hit): prefilter, align and cluster in one '
                                            'process, comparing every genome with the representatives only',
                        formatter_class=fmt, add_help=False)
    io_args(dr, 'Input FASTA file or directory of files (gzipped or uncompressed)')
    db_option(dr)
    prior_options(dr, 'clusters.tsv of an earlier run over the genomes of --db: its clusters and representatives are kept as they '
                      'are, the genomes of -i are added to them, and only its representatives are ever compared (needs --db)')
    prefilter_options(dr, 'the prefilter')
    lz_options(dr)
    cluster_filter_options(dr, default='cd-hit', choices=['cd-hit'],
                           help='Clustering algorithm [%(default)s]: a genome joins the earliest (longest) representative it has a passing '
                                'row to, else it becomes one')
    dr.add_argument('--batch-genomes', metavar='<int>', type=int, dest='batch_genomes', default=None,
                    help='Genomes compared with the representatives at a time; results do not depend on it [4096]')
    dr.add_argument('--out-table', metavar='<file>', type=pathlib.Path, dest='table_path',
                    help='Write the ANI rows that were computed (a subset of the rows of `align`) to the tsv <file>, with its .ids.tsv')
    dr.add_argument('--outfmt', metavar='<str>', choices=ALIGN_OUTFMT.keys(), dest='outfmt', default='standard',
                    help='Format of --out-table [%(default)s]\nchoices: ' + ','.join(ALIGN_OUTFMT.keys()))
    dr.add_argument('--out-repr-fasta', metavar='<file>', type=pathlib.Path, dest='repr_fasta_path',
                    help='Write the records of the representative genomes to the FASTA <file> (a single multi-FASTA input only; '
                         'with --db, one on each side: the records of --db first)')
    common(dr)

    sub.add_parser('info', help='Show information about the tool and its dependencies', formatter_class=fmt,
                   add_help=False)

    # no arguments: help on stdout, exit 0 (test.py:41-55)
    if len(sys.argv[1:]) == 0:
        parser.print_help()
        parser.exit()
    for name, sp in (('prefilter', pf), ('align', al), ('cluster', cl), ('deduplicate', dd), ('dereplicate', dr)):
        if sys.argv[-1] == name:
            sp.print_help()
            parser.exit()
    return parser


# ------------------------------------------------------------------ logging
class _LogFormatter(logging.Formatter):
    FMT = '{asctime} [{levelname:^7}] {message}'
    COLORS = {logging.DEBUG: '{}', logging.INFO: '\33[36m{}\33[0m', logging.WARNING: '\33[33m{}\33[0m',
              logging.ERROR: '\33[31m{}\33[0m'}

    def format(self, record):
        fmt = self.COLORS.get(record.levelno, '{}').replace('{}', self.FMT)
        return logging.Formatter(fmt, style='{').format(record)


def create_logger(name: str, verbosity_level: int) -> logging.Logger:
    level = {0: logging.ERROR, 1: logging.INFO, 2: logging.DEBUG}.get(verbosity_level, logging.ERROR)
    logger = logging.getLogger(name)
    logger.setLevel(level)
    if not logger.handlers:
        handler = logging.StreamHandler()
        handler.setLevel(level)
        handler.setFormatter(_LogFormatter())
        logger.addHandler(handler)
    return logger


# ------------------------------------------------------------------ helpers
def validate_args_fasta_input(args, parser):
    """file -> one multi-FASTA; directory -> one genome per file, sorted, at least two."""
    args.is_multifasta = True
    args.fasta_paths = [args.input_path]
    if args.input_path.is_dir():
        args.is_multifasta = False
        args.fasta_paths = sorted(f for f in args.input_path.iterdir() if f.is_file())
    args.db_paths = None
    db_path = getattr(args, 'db_path', None)
    if db_path is None:
        if not args.is_multifasta and len(args.fasta_paths) < 2:
            parser.error(f'Too few fasta files found in {args.input_path}. '
                         f'Expected at least 2, found {len(args.fasta_paths)}.')
        return args
    # --db: read by the rule of -i; the two are of one kind, and the combined set needs two genomes
    if db_path.is_dir() != args.input_path.is_dir():
        parser.error('-i and --db must both be FASTA files or both be directories.')
    if dist_env()[1] > 1:
        parser.error('--db runs on one GPU: start it without a multi-process launcher (WORLD_SIZE must be 1).')
    args.db_paths = sorted(f for f in db_path.iterdir() if f.is_file()) if db_path.is_dir() else [db_path]
    if not args.is_multifasta:
        for path, found in ((db_path, args.db_paths), (args.input_path, args.fasta_paths)):
            if not found:
                parser.error(f'No fasta files found in {path}.')
    return args


def _db_description(args):
    """The database and the file counts, for the 'Running:' line ('' without --db)."""
    if args.db_paths is None:
        return ''
    return f' --db {args.db_path} [{len(args.db_paths)} database + {len(args.fasta_paths)} new file(s)]'


def validate_args_prefilter(args, parser):
    if args.batch_size and args.input_path.is_dir():
        parser.error('--batch-size only handles a multi-fasta file, not a directory.')
    return args


def _check_prior_pair(args, parser):
    if getattr(args, 'prior_path', None) is None and getattr(args, 'prior_repr', False):
        parser.error('--prior-repr describes the file of --prior: it needs --prior.')


def _check_metric_threshold(args, parser):
    if not vars(args).get(args.metric, 0):
        parser.error(f'{args.metric} threshold must be above 0. Specify the option: --{args.metric}')


def run_native(description, fn, verbosity_level, logger):
    """The reference's run(): log 'Running', call, log 'Completed'; errors -> ERROR log + exit 1."""
    logger.info(f'Running: {description}')
    try:
        fn()
    except Exception as e:      # library error codes arrive as VclustGpuError
        logger.error(f'Process {description} failed with message: {e}')
        sys.exit(1)
    logger.info('Completed')


def run_subprocess(cmd, verbosity_level, logger):
    logger.info(f'Running: {" ".join(cmd)}')
    try:
        subprocess.run(cmd, stdout=None if verbosity_level else subprocess.DEVNULL,
                       stderr=None if verbosity_level else subprocess.PIPE, text=True, check=True)
    except subprocess.CalledProcessError as e:
        logger.error(f'Process {" ".join(cmd)} failed with message: {e.stderr}')
        sys.exit(1)
    except OSError as e:
        logger.error(f'OSError: {" ".join(cmd)} failed with message: {e}')
        sys.exit(1)
    logger.info('Completed')


def _require_binary(path):
    if not path.exists() or not os.access(path, os.X_OK):
        sys.exit(f'error: File not found: {path} (CPU tool, not part of the GPU path; build it from the '
                 'reference repository and place it in bin/)')


# ------------------------------------------------------------------ handlers
def prefilter_call(args):
    """What the front-end hands to vg_prefilter for validated prefilter arguments -- the counterpart of the
    reference's three argv lists (cmd_kmerdb_build / _all2all / _distance, vclust.py:915-1055)."""
    call = dict(paths=args.fasta_paths, out_path=args.output_path, is_multifasta=args.is_multifasta, k=args.k,
                min_kmers=args.min_kmers, min_ident=args.min_ident, kmers_fraction=args.kmers_fraction,
                max_seqs=args.max_seqs, num_threads=args.num_threads)
    if getattr(args, 'db_paths', None) is not None:       # --db: vg_prefilter_new (no reference counterpart)
        call['db_paths'] = args.db_paths
    return call


def align_call(args):
    """What the front-end hands to vg_align for validated align arguments -- the counterpart of cmd_lzani
    (vclust.py:1058-1181): `--out-filter` only for values > 0 (:1170-1176), `--multisample-fasta true` iff there
    is exactly one input path (:1159-1160)."""
    out_filters = {k: getattr(args, k) for k in ('tani', 'gani', 'ani', 'qcov', 'rcov') if getattr(args, k) > 0}
    call = dict(paths=args.fasta_paths, out_path=args.output_path, is_multifasta=args.is_multifasta,
                columns=ALIGN_OUTFMT[args.outfmt], filter_path=args.filter_path, filter_threshold=args.filter_threshold,
                out_aln=args.aln_path, lz=lz_of(args), out_filters=out_filters, num_threads=args.num_threads)
    if getattr(args, 'db_paths', None) is not None:       # --db: vg_align_new (no reference counterpart)
        call['db_paths'] = args.db_paths
    return call


def handle_prefilter(args, parser, logger):
    args = validate_args_prefilter(args, parser)
    args = validate_args_fasta_input(args, parser)
    world = dist_env()[1]
    desc = f'libvclust_gpu prefilter {_prefilter_text(args)} --max-seqs {args.max_seqs}{_db_description(args)} [{world} GPU] -> {args.output_path}'

    def work():
        kw = prefilter_call(args)
        paths, out_path, multi = kw.pop('paths'), kw.pop('out_path'), kw.pop('is_multifasta')
        if world == 1:
            stages.prefilter(paths, out_path, multi, batch_size=args.batch_size, verbosity=args.verbosity_level, **kw)
        else:
            from . import distributed
            distributed.prefilter(paths, out_path, multi, **kw)
    run_native(desc, work, args.verbosity_level, logger)


def handle_align(args, parser, logger):
    args = validate_args_fasta_input(args, parser)
    world = dist_env()[1]
    call = align_call(args)
    desc = ('libvclust_gpu align ' + _lz_text(args)
            + (f' --filter {args.filter_path} {args.filter_threshold}' if args.filter_path else '')
            + _db_description(args) + f' [{world} GPU] -> {args.output_path}')

    def work():
        kw = dict(call)
        paths, out_path, multi = kw.pop('paths'), kw.pop('out_path'), kw.pop('is_multifasta')
        if world == 1:
            stages.align(paths, out_path, multi, verbosity=args.verbosity_level, **kw)
        else:
            from . import distributed
            distributed.align(paths, out_path, multi, **kw)
    run_native(desc, work, args.verbosity_level, logger)


def cluster_call(args):
    """What the front-end hands to vg_cluster for validated cluster arguments -- the counterpart of cmd_clusty
    (vclust.py:1184-1278): a minimum only for values > 0, the num_alns maximum only for values > 0.  With --prior the call
    also carries prior_path and prior_repr, and goes to vg_cluster_update."""
    call = dict(ani_path=args.input_path, ids_path=args.ids_path, out_path=args.output_path, algorithm=args.algorithm,
                metric=args.metric, num_alns=max(args.num_alns, 0), representatives=args.representatives, **minimums_of(args))
    if getattr(args, 'linkage_path', None) is not None:
        call['out_linkage'] = args.linkage_path
    if getattr(args, 'levels', None):
        call['levels'] = list(args.levels)
    if getattr(args, 'prior_path', None) is not None:     # --prior: vg_cluster_update (no reference counterpart)
        call['prior_path'] = args.prior_path
        call['prior_repr'] = bool(args.prior_repr)
    if args.algorithm == 'mcl':                           # Markov clustering: vg_cluster_mcl (no reference counterpart)
        for key in ('mcl_inflation', 'mcl_prune', 'mcl_max_row', 'mcl_iterations'):
            call[key] = getattr(args, key)
    return call


def validate_args_cluster(args, parser):
    """The checks of `cluster`, and who computes it: args.native is set where the library does -- always for the merge table, its
    cuts, average linkage, Markov clustering and --prior, and for single / cd-hit / uclust / set-cover where there is no bin/clusty
    (vg_cluster).  A plain `--algorithm complete` is not in CLUSTER_ALGORITHMS and goes to Clusty, which must
    then exist."""
    linkage_path, levels = getattr(args, 'linkage_path', None), getattr(args, 'levels', None)
    hierarchy = linkage_path is not None or bool(levels)
    prior_path = getattr(args, 'prior_path', None)
    _check_prior_pair(args, parser)
    if prior_path is not None:
        if args.algorithm not in UPDATE_ALGORITHMS:
            parser.error(f'--prior adds genomes to an earlier clustering under --algorithm {", ".join(UPDATE_ALGORITHMS)}, '
                         f'not under {args.algorithm}.')
        if hierarchy:
            parser.error('--prior takes the earlier clusters as given: it excludes --out-linkage and --levels.')
    if hierarchy:
        if args.algorithm not in HIERARCHY_ALGORITHMS:
            parser.error('--out-linkage and --levels are a linkage hierarchy: they need --algorithm single, --algorithm complete '
                         'or --algorithm average.')
        floor = vars(args).get(args.metric, 0)
        for level in levels or ():
            if floor and level < floor:
                parser.error(f'--levels {level:g} is below --{args.metric} {floor:g}: rows below the threshold are not edges.')
    mcl = args.algorithm == 'mcl'
    if mcl:
        if abs(2 * args.mcl_inflation - round(2 * args.mcl_inflation)) >= 1e-9 or not 1.5 <= args.mcl_inflation <= 6:
            parser.error(f'--mcl-inflation {args.mcl_inflation:g} must be a multiple of 0.5 between 1.5 and 6.')
        if not 0 <= args.mcl_prune <= 0.1:
            parser.error(f'--mcl-prune {args.mcl_prune:g} must lie between 0 and 0.1.')
        if not 2 <= args.mcl_max_row <= 4096:
            parser.error(f'--mcl-max-row {args.mcl_max_row} must lie between 2 and 4096.')
        if not 1 <= args.mcl_iterations <= 1000:
            parser.error(f'--mcl-iterations {args.mcl_iterations} must lie between 1 and 1000.')
    args.native = (hierarchy or prior_path is not None or args.algorithm == 'average' or mcl
                   or (not BIN_CLUSTY.exists() and args.algorithm in CLUSTER_ALGORITHMS))
    if not args.native:
        _require_binary(BIN_CLUSTY)
    _check_metric_threshold(args, parser)
    return args


def _cluster_description(args):
    """The library's clustering for the 'Running:' line, in the words of the command line."""
    levels, linkage_path = getattr(args, 'levels', None), getattr(args, 'linkage_path', None)
    return (f'libvclust_gpu cluster --algorithm {args.algorithm}' + (f' --mcl-inflation {args.mcl_inflation:g}' if args.algorithm == 'mcl' else '')
            + _filters_text(args) + (f' --levels {" ".join(f"{x:g}" for x in levels)}' if levels else '')
            + (f' --out-linkage {linkage_path}' if linkage_path is not None else '') + _prior_text(args) + f' [1 GPU] -> {args.output_path}')


def handle_cluster(args, parser, logger):
    """`cluster`: bin/clusty where it exists and computes what is asked, the library otherwise (validate_args_cluster).  --prior adds
    the genomes of --ids that the earlier clusters.tsv does not list to its clusters (the ids file and the rows are those of an
    `align --db` run; DESIGN.md section 9, "Update of a prior clustering")."""
    args = validate_args_cluster(args, parser)
    if args.native:
        call = cluster_call(args)
        counts = []
        run_native(_cluster_description(args), lambda: counts.append(stages.cluster(verbosity=args.verbosity_level, **call)),
                   args.verbosity_level, logger)
        if getattr(args, 'prior_path', None) is not None:
            c = counts[0]
            logger.info(f'Prior clustering updated: {c["n_prior"]} prior + {c["n_new"]} new genomes, {c["n_edges"]} kept edges; new genomes: '
                        f'{c["joined_prior"]} joined a prior cluster, {c["joined_new"]} joined a new one, {c["founded"]} founded a cluster; '
                        f'{c["prior_merged"]} prior cluster(s) merged away')
        if args.algorithm == 'mcl':
            c = counts[0]
            with open(args.output_path) as f:
                labels = {line.split('\t')[1] for line in f.read().split('\n')[1:] if line}
            logger.info(f'MCL: {c["iterations"]} iterations, chaos {c["chaos"] / (1 << 30):.3g}, {len(labels)} clusters')
            if not c['converged']:
                logger.warning(f'MCL did not converge within --mcl-iterations {args.mcl_iterations}: the clusters are those of the last iterate')
        cluster_report(args, logger)
        return
    cmd = [str(BIN_CLUSTY), '--objects-file', str(args.ids_path), '--algo', args.algorithm, '--id-cols', 'qidx', 'ridx',
           '--distance-col', args.metric, '--similarity', '--numeric-ids']
    for name, value in minimums_of(args).items():
        cmd += ['--min', name, str(value)]
    if args.num_alns > 0:
        cmd += ['--max', 'num_alns', str(args.num_alns)]
    if args.representatives:
        cmd.append('--out-representatives')
    if args.algorithm == 'leiden':
        cmd += ['--leiden-resolution', str(args.leiden_resolution), '--leiden-beta', str(args.leiden_beta),
                '--leiden-iterations', str(args.leiden_iterations)]
    cmd += [str(args.input_path), str(args.output_path)]
    run_subprocess(cmd, args.verbosity_level, logger)
    cluster_report(args, logger)


def cluster_stats_call(args):
    """What the front-end hands to vg_cluster_stats_file for validated cluster arguments: the filters and the metric of the
    clustering itself (cluster_call), the clusters.tsv just written, and whether it holds representative ids."""
    return dict(ani_path=args.input_path, ids_path=args.ids_path, clusters_path=args.output_path, out_path=args.stats_path,
                clusters_repr=bool(args.representatives), metric=args.metric, num_alns=max(args.num_alns, 0), **minimums_of(args))


def cluster_report(args, logger):
    """--out-stats: the second call of `cluster`, made once clusters.tsv is complete -- whoever wrote it, the library or
    bin/clusty ("Cluster report").  It always runs in the library, under a `Running:` / `Completed` pair of
    its own."""
    if getattr(args, 'stats_path', None) is None:
        return
    call = cluster_stats_call(args)
    desc = f'libvclust_gpu cluster-stats{_filters_text(args)} --clusters {args.output_path} [1 GPU] -> {args.stats_path}'
    run_native(desc, lambda: stages.cluster_stats(verbosity=args.verbosity_level, **call), args.verbosity_level, logger)


def validate_args_deduplicate(args, parser):
    """The reference's checks and defaults (validate_args_deduplicate, vclust.py:705-728): one prefix per file and no
    comma in any, a bare --add-prefixes means `<file stem before the first '.'>|`, a gzip level in 1..9, `.gz` added to
    the output name under --gzip-output, and the duplicates file `<output>.duplicates.txt`.  Directories are not FASTA
    files here."""
    for f in args.input_path:
        if f.is_dir():
            parser.error(f'{f} is a directory; deduplicate takes FASTA files')
    if args.add_prefixes:
        if len(args.add_prefixes) != len(args.input_path):
            parser.error('Number of prefixes must match the number of input files.')
        if any(',' in prefix for prefix in args.add_prefixes):
            parser.error('Prefixes cannot contain commas.')
    elif args.add_prefixes == []:
        args.add_prefixes = [f'{f.stem.split(".")[0]}|' for f in args.input_path]
    if not (1 <= args.gzip_level <= 9):
        parser.error('Compression level must be between 1 and 9.')
    if args.gzip_output and not args.output_path.suffix == '.gz':
        args.output_path = pathlib.Path(f'{args.output_path}.gz')
    args.output_duplicates_path = pathlib.Path(f'{args.output_path}.duplicates.txt')
    return args


def deduplicate_call(args):
    """What the front-end hands to vg_deduplicate for validated deduplicate arguments."""
    return dict(paths=args.input_path, out_path=args.output_path, dup_path=args.output_duplicates_path,
                prefixes=args.add_prefixes or None, gzip_level=args.gzip_level if args.gzip_output else 0,
                num_threads=args.num_threads)


def handle_deduplicate(args, parser, logger):
    circular = getattr(args, 'circular', False)
    contained = getattr(args, 'contained', False)
    if circular and contained:
        parser.error('--contained and --circular exclude each other.')
    terminal_repeat = getattr(args, 'terminal_repeat', None)
    if terminal_repeat is not None and not circular:
        parser.error('--terminal-repeat needs --circular.')
    if terminal_repeat is not None and terminal_repeat < 1:
        parser.error('--terminal-repeat must be at least 1.')
    if circular or contained or not BIN_MFASTA.exists():
        # no mfasta-tool, or --circular / --contained (which mfasta-tool does not have): the GPU (vg_deduplicate)
        args = validate_args_deduplicate(args, parser)
        call = deduplicate_call(args)
        desc = (f'libvclust_gpu deduplicate -i {" ".join(str(f) for f in args.input_path)}'
                + (f' --add-prefixes {" ".join(args.add_prefixes)}' if args.add_prefixes else '')
                + (f' --gzip-level {args.gzip_level}' if args.gzip_output else '')
                + (' --circular' if circular else '')
                + (f' --terminal-repeat {terminal_repeat}' if terminal_repeat is not None else '')
                + (' --contained' if contained else '')
                + f' [1 GPU] -> {args.output_path}, {args.output_duplicates_path}')
        if circular:
            call['circular'] = True
        if terminal_repeat is not None:
            call['terminal_repeat'] = terminal_repeat
        if contained:
            call['contained'] = True
        run_native(desc, lambda: stages.deduplicate(verbosity=args.verbosity_level, **call), args.verbosity_level, logger)
        return
    _require_binary(BIN_MFASTA)
    out_dup = pathlib.Path(f'{args.output_path}.duplicates.txt')
    cmd = [str(BIN_MFASTA), 'mrds', '-i', ','.join(str(f) for f in args.input_path), '-o', str(args.output_path),
           '--out-duplicates', str(out_dup), '--remove-duplicates', '--mark-duplicates-orientation',
           '--rev-comp-as-equivalent', '-t', str(args.num_threads)]
    if args.verbosity_level:
        cmd += ['--verbosity', '1']
    if args.add_prefixes:
        cmd += ['--in-prefixes', ','.join(args.add_prefixes)]
    if args.gzip_output:
        cmd += ['--gzipped-output', '--gzip-level', str(args.gzip_level)]
    run_subprocess(cmd, args.verbosity_level, logger)


def dereplicate_call(args):
    """What the front-end hands to vg_dereplicate for validated dereplicate arguments: the prefilter, align and cluster options as
    prefilter_call, align_call and cluster_call pass them."""
    call = dict(paths=args.fasta_paths, out_path=args.output_path, is_multifasta=args.is_multifasta, batch_genomes=args.batch_genomes,
                k=args.k, kmers_fraction=args.kmers_fraction, min_kmers=args.min_kmers, min_ident=args.min_ident, lz=lz_of(args),
                algorithm=args.algorithm, metric=args.metric, num_alns=max(args.num_alns, 0), representatives=args.representatives,
                out_table=args.table_path, columns=ALIGN_OUTFMT[args.outfmt], out_repr_fasta=args.repr_fasta_path,
                num_threads=args.num_threads, **minimums_of(args))
    if getattr(args, 'db_paths', None) is not None:       # --db --prior: vg_dereplicate_update
        call.update(db_paths=args.db_paths, prior_path=args.prior_path, prior_repr=bool(args.prior_repr))
    return call


def handle_dereplicate(args, parser, logger):
    """`dereplicate`: prefilter -> align -> cluster --algorithm cd-hit in one process, batch by batch against the representatives
    (vg_dereplicate).  With --db and --prior the genomes of -i are added to the clusters of an earlier run
    over --db (vg_dereplicate_update).  Always in the library; one GPU."""
    prior_path, db_path = getattr(args, 'prior_path', None), getattr(args, 'db_path', None)
    _check_prior_pair(args, parser)
    if prior_path is not None and db_path is None:
        parser.error('--prior names the clusters of the genomes of --db: it needs --db.')
    if db_path is not None and prior_path is None:
        parser.error('--db holds the genomes of an earlier run: it needs the clusters.tsv of that run as --prior.')
    args = validate_args_fasta_input(args, parser)
    if dist_env()[1] > 1:
        parser.error('dereplicate runs on one GPU: start it without a multi-process launcher (WORLD_SIZE must be 1).')
    _check_metric_threshold(args, parser)
    if args.batch_genomes is not None and args.batch_genomes < 1:
        parser.error('--batch-genomes must be at least 1.')
    if args.repr_fasta_path is not None and not args.is_multifasta:
        parser.error('--out-repr-fasta copies the records of one multi-FASTA file: it does not take a directory input.')
    call = dereplicate_call(args)
    desc = (f'libvclust_gpu dereplicate {_prefilter_text(args)} {_lz_text(args)} --algorithm {args.algorithm}{_filters_text(args)}'
            + (f' --batch-genomes {args.batch_genomes}' if args.batch_genomes is not None else '')
            + (f' --out-table {args.table_path}' if args.table_path is not None else '')
            + (f' --out-repr-fasta {args.repr_fasta_path}' if args.repr_fasta_path is not None else '')
            + _db_description(args) + _prior_text(args) + f' [1 GPU] -> {args.output_path}')
    run_native(desc, lambda: stages.dereplicate(verbosity=args.verbosity_level, **call), args.verbosity_level, logger)


def handle_info(args, parser, logger):
    lines = [f'Vclust (MI355X-native prefilter/align) version {__version__}', '', 'GPU path:']
    ok = True
    try:
        from . import api
        lines.append(f'   libvclust_gpu        {api.version()}')
        n = api.device_count()
        lines.append(f'   HIP devices          {n}')
        ok = n > 0
    except Exception as e:      # noqa: BLE001
        lines.append(f'   libvclust_gpu        [error] {e}')
        ok = False
    lines += ['', 'Parity with the reference (golden example of refresh-bio/vclust, DESIGN.md section 2):',
              '   fltr.txt, ani.ids.tsv            byte-identical',
              '   ani.aln.tsv                      5693 / 5693 regions identical, none surplus',
              '   ani.tsv                          132 / 132 rows byte-identical']
    lines += ['', 'CPU tools (optional):']
    for name, path in (('Clusty', BIN_CLUSTY), ('mfasta', BIN_MFASTA)):
        lines.append(f'   {name:<20} {"found" if path.exists() else "not installed"} ({path})')
    lines += ['', '\033[32;1mStatus: ready\033[0m' if ok else '\033[31mStatus: error\033[0m']
    print('\n'.join(lines))
    if not ok:
        sys.exit(1)


def main():
    parser = get_parser()
    args = parser.parse_args()
    rank = dist_env()[0]
    logger = create_logger('Vclust', getattr(args, 'verbosity_level', 0) if rank == 0 else 0)
    handlers = {'info': handle_info, 'deduplicate': handle_deduplicate, 'prefilter': handle_prefilter,
                'align': handle_align, 'cluster': handle_cluster, 'dereplicate': handle_dereplicate}
    if args.command in handlers:
        handlers[args.command](args, parser, logger)


if __name__ == '__main__':
    main()
