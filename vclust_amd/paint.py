"""Mosaic painting of an alignment table: per position of every genome the partner of the highest identity, as the maximal runs of
one winning alignment, with the per-genome summary and the donor table (vg_paint_file).

    python -m vclust_amd.paint -i ani.aln.tsv --ids ani.ids.tsv -o paint.tsv [--clusters clusters.tsv [--clusters-repr]
                               [--column NAME]] [--out-segments FILE] [--out-donors FILE] [-t N] [-v N]

A command module of its own, as vclust_amd.cover is: vclust.py gets no option.  It imports neither numpy nor torch; the whole run
is one library call.
"""
import argparse
import pathlib
import sys

from . import stages
from .cli import DEFAULT_THREAD_COUNT, create_logger, run_native


def get_parser():
    p = argparse.ArgumentParser(prog='python -m vclust_amd.paint', description='The closest partner of every genome at every position (GPU).')
    p.add_argument('-i', '--in', metavar='<file>', type=pathlib.Path, dest='aln_path', required=True,
                   help='Alignment table written by `vclust.py align --out-aln` (columns query, reference, alnlen, qstart, qend, nt_match)')
    p.add_argument('--ids', metavar='<file>', type=pathlib.Path, dest='ids_path', required=True,
                   help='The ids file of that run (ani.ids.tsv: columns id, seq_len)')
    p.add_argument('-o', '--out', metavar='<file>', type=pathlib.Path, dest='out_path', required=True,
                   help='Output: one line per genome')
    p.add_argument('--clusters', metavar='<file>', type=pathlib.Path, dest='clusters_path',
                   help='A clusters.tsv of the same genomes: painted positions are split into partners of the own cluster and others')
    p.add_argument('--clusters-repr', action='store_true', help='The label columns of --clusters hold representative ids')
    p.add_argument('--column', metavar='<str>', help='The label column of --clusters to use [the first]')
    p.add_argument('--out-segments', metavar='<file>', type=pathlib.Path, dest='segments_path',
                   help='Also write the painting: one line per maximal run of one winning alignment')
    p.add_argument('--out-donors', metavar='<file>', type=pathlib.Path, dest='donors_path',
                   help='Also write the donor table: one line per genome and winning partner')
    p.add_argument('-t', '--threads', metavar='<int>', type=int, dest='num_threads', default=DEFAULT_THREAD_COUNT,
                   help='Number of host threads [%(default)s]')
    p.add_argument('-v', metavar='<int>', type=int, dest='verbosity_level', choices=[0, 1, 2], default=1,
                   help='Verbosity level [%(default)s]')
    return p


def main(argv=None):
    parser = get_parser()
    args = parser.parse_args(argv)
    if args.clusters_path is None and (args.clusters_repr or args.column is not None):
        parser.error('--clusters-repr and --column describe the file of --clusters: they need --clusters.')
    if args.num_threads < 0:
        parser.error('-t must not be negative.')
    for opt, path in (('-i', args.aln_path), ('--ids', args.ids_path), ('--clusters', args.clusters_path)):
        if path is not None and not path.is_file():
            parser.error(f'{opt}: {path} is not a file.')
    logger = create_logger('vclust_amd.paint', args.verbosity_level)
    description = f'libvclust_gpu paint -i {args.aln_path} --ids {args.ids_path} -o {args.out_path}' + \
        (f' --clusters {args.clusters_path}' if args.clusters_path else '') + (f' --column {args.column}' if args.column else '') + \
        (f' --out-segments {args.segments_path}' if args.segments_path else '') + (f' --out-donors {args.donors_path}' if args.donors_path else '')
    run_native(description, lambda: stages.paint(
        args.aln_path, args.ids_path, args.out_path, clusters_path=args.clusters_path, clusters_repr=args.clusters_repr, column=args.column,
        segments_path=args.segments_path, donors_path=args.donors_path, num_threads=args.num_threads, verbosity=args.verbosity_level),
        args.verbosity_level, logger)


if __name__ == '__main__':
    sys.exit(main())
