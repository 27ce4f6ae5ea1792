#!/usr/bin/env python3
"""Fixture generator: records what the Python front end (vclust_amd/cli.py, stages.py, api.py, _lib.py, distributed.py) shows to
its users and hands to the library, without a device and without the built library.  The result, tests/golden/python_surface.json,
pins that surface for tests/test_python_surface_cpu.py, which recomputes surface() and compares.

  * CLI leg: the help text of every parser; for a list of command lines, the keyword arguments that reach the stage functions
    (replaced by recorders) and every log record; for every usage error, the message and the exit status.
  * C-call leg: vclust_amd._lib._lib is a stand-in that records each call by symbol, with the arguments rendered by value
    (structures by field, byref() by its object, path arrays by content, numpy-backed pointers by the array's dtype, shape and content) and returns 0; every
    public function of stages, api and the array-level functions of distributed is called through it, and the calls, the returned
    Python values and the ValueError / TypeError messages are recorded.  The record dtypes are recorded by descr and itemsize.

Paths are replaced by <GOLDEN> (tests/golden/example) and <TMP>.

    python tools/make_python_surface.py
"""
import contextlib
import ctypes as C
import io
import json
import logging
import os
import pathlib
import sys
import tempfile
from unittest import mock

ROOT = pathlib.Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

from vclust_amd import _lib, api, cli, distributed, stages  # noqa: E402

GOLDEN = ROOT / 'tests' / 'golden' / 'example'
FIXTURE = ROOT / 'tests' / 'golden' / 'python_surface.json'
SUBCOMMANDS = ('deduplicate', 'prefilter', 'align', 'cluster', 'dereplicate', 'info')

F, FGZ, DIR = '<GOLDEN>/multifasta.fna', '<GOLDEN>/multifasta.fna.gz', '<GOLDEN>/fna'
ANI, IDS, PRIOR, FLTR = (f'<GOLDEN>/output/{x}' for x in ('ani.tsv', 'ani.ids.tsv', 'clusters.tsv', 'fltr.txt'))
LZ = ['--mal', '14', '--msl', '8', '--mrd', '60', '--mqd', '70', '--reg', '50', '--aw', '25', '--am', '12', '--ar', '4']
MINS = ['--tani', '0.9', '--gani', '0.8', '--ani', '0.95', '--qcov', '0.85', '--rcov', '0.7', '--len_ratio', '0.6', '--num_alns', '5']
CL = ['cluster', '-i', ANI, '--ids', IDS, '-o', '<TMP>/clusters.tsv']
DD = ['deduplicate', '-o', '<TMP>/out.fna', '-i']
DR = ['dereplicate', '-i', F, '-o', '<TMP>/derep.tsv']
W2 = {'WORLD_SIZE': '2', 'RANK': '0', 'LOCAL_RANK': '0'}

# (command line, environment) -- every option of every subcommand at least once
CLI_CASES = [
    (DD + [F], None),
    (DD + [F, FGZ, '--add-prefixes'], None),
    (DD + [F, FGZ, '--add-prefixes', 'a|', 'b|', '--gzip-output', '--gzip-level', '6', '-t', '3', '-v', '2'], None),
    (DD + [FGZ, '--gzip-output'], None),
    (DD + [F, '--circular'], None),
    (DD + [F, '--circular', '--terminal-repeat', '10'], None),
    (DD + [F, '--contained', '-v', '0'], None),
    (['prefilter', '-i', F, '-o', '<TMP>/fltr.txt'], None),
    (['prefilter', '-i', DIR, '-o', '<TMP>/fltr.txt', '-k', '20', '--min-kmers', '30', '--min-ident', '0.9', '--kmers-fraction', '0.5',
      '--max-seqs', '5', '-t', '3', '-v', '2'], None),
    (['prefilter', '-i', F, '-o', '<TMP>/fltr.txt', '--batch-size', '100'], None),
    (['prefilter', '-i', F, '-o', '<TMP>/fltr.txt', '--db', FGZ, '--max-seqs', '2'], None),
    (['prefilter', '-i', DIR, '-o', '<TMP>/fltr.txt', '--db', DIR], None),
    (['prefilter', '-i', F, '-o', '<TMP>/fltr.txt', '-k', '18', '-t', '2'], W2),
    (['align', '-i', F, '-o', '<TMP>/ani.tsv'], None),
    (['align', '-i', DIR, '-o', '<TMP>/ani.tsv', '--filter', FLTR, '--filter-threshold', '0.8', '--outfmt', 'complete', '--out-aln',
      '<TMP>/aln.tsv', '--out-ani', '0.95', '--out-tani', '0.7', '--out-gani', '0.6', '--out-qcov', '0.85', '--out-rcov', '0.5', '-t', '5',
      '-v', '2'] + LZ, None),
    (['align', '-i', F, '-o', '<TMP>/ani.tsv', '--outfmt', 'lite', '--out-ani', '0'], None),
    (['align', '-i', F, '-o', '<TMP>/ani.tsv', '--db', FGZ, '--filter', FLTR], None),
    (['align', '-i', F, '-o', '<TMP>/ani.tsv', '--filter', FLTR, '--filter-threshold', '0.5', '--out-aln', '<TMP>/aln.tsv', '--mal', '12'], W2),
    (CL + ['--tani', '0.95'], None),
    (CL + ['--algorithm', 'cd-hit', '--metric', 'ani', '-r', '-v', '2'] + MINS, None),
    (CL + ['--algorithm', 'uclust', '--metric', 'gani', '--gani', '0.9', '--num_alns', '-3'], None),
    (CL + ['--tani', '0.95', '--out-linkage', '<TMP>/linkage.tsv', '--levels', '0.96', '0.98'], None),
    (CL + ['--algorithm', 'complete', '--tani', '0.95', '--levels', '0.97', '-r'], None),
    (CL + ['--algorithm', 'average', '--metric', 'ani', '--ani', '0.9', '--out-linkage', '<TMP>/linkage.tsv'], None),
    (CL + ['--algorithm', 'average', '--tani', '0.9'], None),
    (CL + ['--algorithm', 'uclust', '--tani', '0.95', '--prior', PRIOR], None),
    (CL + ['--algorithm', 'cd-hit', '--tani', '0.95', '--qcov', '0.5', '--prior', PRIOR, '--prior-repr', '-r'], None),
    (CL + ['--algorithm', 'mcl', '--tani', '0.95'], None),
    (CL + ['--algorithm', 'mcl', '--tani', '0.95', '--mcl-inflation', '2.5', '--mcl-prune', '0.001', '--mcl-max-row', '64', '--mcl-iterations', '7',
           '-r'], None),
    (CL + ['--algorithm', 'set-cover', '--tani', '0.95', '--rcov', '0.5', '--num_alns', '4', '-r', '--out-stats', '<TMP>/stats.tsv'], None),
    (CL + ['--algorithm', 'leiden', '--tani', '0.95', '--leiden-resolution', '0.8', '--leiden-beta', '0.02', '--leiden-iterations', '3'], None),
    (CL + ['--algorithm', 'complete', '--tani', '0.95'], None),
    (DR + ['--tani', '0.95'], None),
    (['dereplicate', '-i', DIR, '-o', '<TMP>/derep.tsv', '-k', '20', '--min-kmers', '30', '--min-ident', '0.9', '--kmers-fraction', '0.5',
      '--algorithm', 'cd-hit', '--metric', 'ani', '-r', '--batch-genomes', '7', '--out-table', '<TMP>/table.tsv', '--outfmt', 'complete', '-t', '3',
      '-v', '2'] + LZ + MINS, None),
    (DR + ['--tani', '0.95', '--out-repr-fasta', '<TMP>/repr.fna', '--outfmt', 'lite', '--out-table', '<TMP>/table.tsv'], None),
    (DR + ['--tani', '0.95', '--db', FGZ, '--prior', PRIOR], None),
    (DR + ['--tani', '0.95', '--ani', '0.9', '--db', FGZ, '--prior', PRIOR, '--prior-repr', '-r', '--msl', '8'], None),
    (['info'], None),
]

# one command line for every parser.error of cli.py, and three that argparse itself refuses
CLI_ERRORS = [
    (['prefilter', '-i', '<TMP>/one', '-o', '<TMP>/x'], None),
    (['prefilter', '-i', F, '-o', '<TMP>/x', '--db', DIR], None),
    (['align', '-i', F, '-o', '<TMP>/x', '--db', FGZ], W2),
    (['align', '-i', DIR, '-o', '<TMP>/x', '--db', '<TMP>/empty'], None),
    (['prefilter', '-i', '<TMP>/empty', '-o', '<TMP>/x', '--db', DIR], None),
    (['prefilter', '-i', DIR, '-o', '<TMP>/x', '--batch-size', '10'], None),
    (CL + ['--tani', '0.95', '--prior-repr'], None),
    (CL + ['--tani', '0.95', '--algorithm', 'set-cover', '--prior', PRIOR], None),
    (CL + ['--tani', '0.95', '--prior', PRIOR, '--levels', '0.97'], None),
    (CL + ['--tani', '0.95', '--algorithm', 'cd-hit', '--out-linkage', '<TMP>/l.tsv'], None),
    (CL + ['--tani', '0.95', '--levels', '0.9'], None),
    (CL + ['--tani', '0.95', '--algorithm', 'mcl', '--mcl-inflation', '2.2'], None),
    (CL + ['--tani', '0.95', '--algorithm', 'mcl', '--mcl-prune', '0.5'], None),
    (CL + ['--tani', '0.95', '--algorithm', 'mcl', '--mcl-max-row', '1'], None),
    (CL + ['--tani', '0.95', '--algorithm', 'mcl', '--mcl-iterations', '0'], None),
    (CL + ['--metric', 'ani', '--tani', '0.95'], None),
    (DD + [DIR], None),
    (DD + [F, FGZ, '--add-prefixes', 'a|'], None),
    (DD + [F, '--add-prefixes', 'a,b'], None),
    (DD + [F, '--gzip-level', '10'], None),
    (DD + [F, '--circular', '--contained'], None),
    (DD + [F, '--terminal-repeat', '10'], None),
    (DD + [F, '--circular', '--terminal-repeat', '0'], None),
    (DR + ['--tani', '0.95', '--prior-repr'], None),
    (DR + ['--tani', '0.95', '--prior', PRIOR], None),
    (DR + ['--tani', '0.95', '--db', FGZ], None),
    (DR + ['--tani', '0.95'], W2),
    (DR + ['--metric', 'gani', '--tani', '0.95'], None),
    (DR + ['--tani', '0.95', '--batch-genomes', '0'], None),
    (['dereplicate', '-i', DIR, '-o', '<TMP>/x', '--tani', '0.95', '--out-repr-fasta', '<TMP>/r.fna'], None),
    (['prefilter', '-i', '<TMP>/missing', '-o', '<TMP>/x'], None),
    (['align', '-i', F, '-o', '<TMP>/x', '--out-ani', '1.5'], None),
    (['dereplicate', '-i', F, '-o', '<TMP>/x', '--algorithm', 'single'], None),
]

COUNTS = dict(n_prior=10, n_new=2, n_edges=31, joined_prior=1, joined_new=0, founded=1, prior_merged=0, iterations=12, converged=1, chaos=1 << 20)


def _plain(x):
    """A recorded value as JSON data: paths as strings, tuples as lists."""
    if isinstance(x, dict):
        return {str(k): _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    if isinstance(x, pathlib.PurePath):
        return str(x)
    return x


def _normalise(x, repl):
    if isinstance(x, dict):
        return {k: _normalise(v, repl) for k, v in x.items()}
    if isinstance(x, list):
        return [_normalise(v, repl) for v in x]
    if isinstance(x, str):
        for path, name in repl:
            x = x.replace(path, name)
    return x


# ------------------------------------------------------------------ CLI leg
class _ListHandler(logging.Handler):
    def __init__(self, records):
        super().__init__(logging.DEBUG)
        self.records = records

    def emit(self, record):
        self.records.append([record.levelname, record.getMessage()])


def _parser(argv):
    with mock.patch.object(sys, 'argv', ['vclust.py'] + argv):
        return cli.get_parser()


def _run_cli(argv, env, tmp):
    """One command line through its handler: the stage calls that arrive, the log records, and how it ends."""
    argv = [a.replace('<GOLDEN>', str(GOLDEN)).replace('<TMP>', str(tmp)) for a in argv]
    calls, logs = [], []
    counts = dict(COUNTS, converged=0) if '7' in argv else dict(COUNTS)        # (--mcl-iterations 7: the run that does not converge)

    def recorder(name):
        def stage(*args, **kw):
            calls.append([name, _plain(args), _plain(kw)])
            if name == 'stages.cluster':
                pathlib.Path(kw['out_path']).write_text('object\tcluster\nA\t0\nB\t1\n')
            return dict(counts)
        return stage

    logger = logging.getLogger('python_surface')
    logger.setLevel(logging.DEBUG)
    logger.propagate = False
    handler = _ListHandler(logs)
    logger.addHandler(handler)
    out = {'argv': argv}
    if env:
        out['env'] = env
    clean = {k: v for k, v in os.environ.items() if k not in W2}
    stderr, stdout = io.StringIO(), io.StringIO()
    try:
        with contextlib.ExitStack() as stack:
            for name in ('prefilter', 'align', 'cluster', 'cluster_stats', 'deduplicate', 'dereplicate'):
                stack.enter_context(mock.patch.object(stages, name, recorder(f'stages.{name}')))
            for name in ('prefilter', 'align'):
                stack.enter_context(mock.patch.object(distributed, name, recorder(f'distributed.{name}')))
            stack.enter_context(mock.patch.object(api, 'version', lambda: 'stand-in'))
            stack.enter_context(mock.patch.object(api, 'device_count', lambda: 1))
            stack.enter_context(mock.patch.dict(os.environ, dict(clean, **(env or {})), clear=True))
            stack.enter_context(mock.patch.object(sys, 'argv', ['vclust.py'] + argv))
            stack.enter_context(contextlib.redirect_stderr(stderr))
            stack.enter_context(contextlib.redirect_stdout(stdout))
            parser = cli.get_parser()
            args = parser.parse_args(argv)
            getattr(cli, f'handle_{args.command}')(args, parser, logger)
    except SystemExit as e:
        out['exit'] = e.code
        out['stderr'] = (stderr.getvalue().strip().splitlines() or [''])[-1]
    finally:
        logger.removeHandler(handler)
    out['calls'], out['log'] = calls, logs
    if stdout.getvalue():
        out['stdout'] = stdout.getvalue()
    return out


def cli_surface():
    helps, cases, errors = {}, [], []
    with contextlib.ExitStack() as stack:
        stack.enter_context(mock.patch.object(cli, 'DEFAULT_THREAD_COUNT', 8))
        stack.enter_context(mock.patch.object(cli, 'BIN_CLUSTY', pathlib.Path('/nonexistent/bin/clusty')))
        stack.enter_context(mock.patch.object(cli, 'BIN_MFASTA', pathlib.Path('/nonexistent/bin/mfasta-tool')))
        tmp = pathlib.Path(stack.enter_context(tempfile.TemporaryDirectory()))
        (tmp / 'one').mkdir()
        (tmp / 'one' / 'a.fna').write_text('>a\nACGT\n')
        (tmp / 'empty').mkdir()
        parser = _parser(['-h', 'x'])
        helps['vclust'] = parser.format_help()
        choices = parser._subparsers._group_actions[0].choices
        for name in SUBCOMMANDS:
            helps[name] = choices[name].format_help()
        repl = [(str(tmp), '<TMP>'), (str(GOLDEN), '<GOLDEN>')]
        cases = [_normalise(_run_cli(argv, env, tmp), repl) for argv, env in CLI_CASES]
        errors = [_normalise(_run_cli(argv, env, tmp), repl) for argv, env in CLI_ERRORS]
    return helps, cases, errors


# ------------------------------------------------------------------ C-call leg
def _render_struct(s):
    out = {}
    for name, t in s._fields_:
        v = getattr(s, name)
        if isinstance(v, C.Structure):
            out[name] = _render_struct(v)
        elif isinstance(v, bytes):
            out[name] = v.decode('utf-8', 'replace')
        elif isinstance(v, C._Pointer):
            count = getattr(s, f'n_{name}', None)
            if v and t is C.POINTER(C.c_char_p) and count is not None:
                out[name] = [v[i].decode() for i in range(count)]
            else:
                out[name] = 'set' if v else 'null'
        else:
            out[name] = v
    return out


def _render_object(o):
    if isinstance(o, C.Structure):
        return _render_struct(o)
    if isinstance(o, C.Array):
        if o._type_ is C.c_char_p:
            return [None if x is None else x.decode('utf-8', 'replace') for x in o]
        if issubclass(o._type_, C._SimpleCData):
            return list(o)
        return {'array': o._type_.__name__, 'n': len(o)}
    if isinstance(o, C._Pointer):
        return 'set' if o else 'null'
    if isinstance(o, C.c_void_p):
        return 'set' if o.value else 'null'
    if isinstance(o, C._SimpleCData):
        return o.value.decode() if isinstance(o.value, bytes) else o.value
    return repr(type(o))


def _render_array(arr):
    dtype = arr.dtype.str if arr.dtype.names is None else [list(d) for d in arr.dtype.descr]
    return {'dtype': dtype, 'shape': list(arr.shape), 'data': arr.tolist()}


def _render_arg(a):
    if a is None or isinstance(a, (bool, int, float)):
        return a
    if isinstance(a, bytes):
        return a.decode('utf-8', 'replace')
    if hasattr(a, '_obj'):                                # byref()
        return {'ref': _render_object(a._obj)}
    arr = getattr(a, '_arr', None)                        # a pointer made by ndarray.ctypes.data_as keeps its array here
    if arr is not None:
        return _render_array(arr)
    return _render_object(a)


class _StandIn:
    """In place of the loaded library: every symbol of _lib.SYMBOLS, each call checked against its argument types and recorded.
    vg_genomes_count, the getter behind len(), is answered (3 genomes) but not recorded: how often a wrapper asks for the length is
    not part of the surface."""
    RETURNS = {'vg_genomes_count': 3}

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        res, argtypes = _lib.SYMBOLS[name]

        def call(*args):
            if len(args) != len(argtypes):
                raise TypeError(f'{name}: {len(args)} arguments for {len(argtypes)}')
            for a, t in zip(args, argtypes):
                t.from_param(a)                           # what ctypes itself would refuse
            if name in self.RETURNS:
                return self.RETURNS[name]
            self.calls.append([name] + [_render_arg(a) for a in args])
            return None if res is None else b'stand-in' if res is C.c_char_p else res().value
        return call


def _render_value(v):
    if isinstance(v, np.ndarray):
        return _render_array(v)
    if isinstance(v, (C.Structure, C.Array)):
        return _render_object(v)
    if isinstance(v, dict):
        return {str(k): _render_value(x) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_render_value(x) for x in v]
    if isinstance(v, (np.integer, np.floating)):
        return v.item()
    if isinstance(v, api.GenomeSet):
        return 'GenomeSet'
    return v


def c_call_surface():
    lib = _StandIn()
    out = []

    def case(label, fn):
        lib.calls = []
        try:
            ret = _render_value(fn())
        except (ValueError, TypeError, IndexError) as e:
            ret = {'raises': type(e).__name__, 'message': str(e)}
        out.append({'case': label, 'c': lib.calls, 'ret': ret})

    P2, DB2 = ['a.fna', pathlib.Path('b.fna')], ['db1.fna', 'db2.fna']
    lz = dict(mal=14, msl=8, mrd=60, mqd=70, reg=50, aw=25, am=12, ar=4)
    cols = ['qidx', 'ridx', 'ani']
    mins = dict(tani=0.9, gani=0.8, ani=0.95, qcov=0.85, rcov=0.7, len_ratio=0.6)
    q, r, w = [0, 1, 2], [1, 2, 0], [0.9, 0.8, 0.7]
    big = 1 << 31
    pairs = np.array([(1, 0, 40), (2, 1, 25)], dtype=api.PAIR_DTYPE)
    tasks = np.array([(0, 1), (1, 0), (2, 1)], dtype=api.TASK_DTYPE)
    rows = np.array([(100, 120, 2), (90, 110, 1), (5, 6, 1)], dtype=api.STAT_DTYPE)
    regions = np.array([(0, 1, 50, 2, 51, 49)], dtype=api.REGION_DTYPE)
    seqs = ['ACGT', b'acgtt', 'GG CC']
    with mock.patch.object(_lib, '_lib', lib):
        # ---- stages
        case('stages.prefilter', lambda: stages.prefilter(P2, 'out.txt', False, k=20, min_kmers=5, min_ident=0.5, batch_size=10, kmers_fraction=0.5,
                                                          max_seqs=3, num_threads=4, verbosity=2))
        case('stages.prefilter db', lambda: stages.prefilter(P2[:1], 'out.txt', True, db_paths=DB2))
        case('stages.align_params', lambda: stages.align_params(cols, 'f.txt', 0.8, 'aln.tsv', lz, dict(ani=0.9, qcov=0.5), 4, 2, False))
        case('stages.align_params defaults', lambda: stages.align_params(cols))
        case('stages.align', lambda: stages.align(P2, 'ani.tsv', False, cols, filter_path='f.txt', filter_threshold=0.8, out_aln='aln.tsv', lz=lz,
                                                  out_filters=dict(tani=0.1, gani=0.2, ani=0.3, qcov=0.4, rcov=0.5), num_threads=4, verbosity=2))
        case('stages.align db', lambda: stages.align(P2[:1], 'ani.tsv', True, cols, lz=dict(msl=8), db_paths=DB2))
        case('stages.cluster', lambda: stages.cluster('ani.tsv', 'ids.tsv', 'c.tsv', algorithm='set-cover', metric='ani', num_alns=5, representatives=True,
                                                      num_threads=4, verbosity=2, **mins))
        case('stages.cluster complete', lambda: stages.cluster('ani.tsv', 'ids.tsv', 'c.tsv', algorithm='complete', tani=0.9))
        case('stages.cluster prior', lambda: stages.cluster('ani.tsv', 'ids.tsv', 'c.tsv', algorithm='uclust', prior_path='p.tsv', prior_repr=True, tani=0.9))
        case('stages.cluster mcl', lambda: stages.cluster('ani.tsv', 'ids.tsv', 'c.tsv', algorithm='mcl', tani=0.9, mcl_inflation=2.5, mcl_prune=1e-3,
                                                          mcl_max_row=64, mcl_chaos_eps=1e-2, mcl_iterations=7))
        case('stages.cluster mcl defaults', lambda: stages.cluster('ani.tsv', 'ids.tsv', 'c.tsv', algorithm='mcl', tani=0.9))
        case('stages.cluster linkage', lambda: stages.cluster('ani.tsv', 'ids.tsv', 'c.tsv', algorithm='average', out_linkage='l.tsv', levels=[0.95, 0.97],
                                                              tani=0.9))
        case('stages.cluster levels', lambda: stages.cluster('ani.tsv', 'ids.tsv', 'c.tsv', levels=[0.95], tani=0.9))
        case('stages.cluster out_linkage', lambda: stages.cluster('ani.tsv', 'ids.tsv', 'c.tsv', algorithm='complete', out_linkage='l.tsv', tani=0.9))
        case('stages.cluster_stats', lambda: stages.cluster_stats('ani.tsv', 'ids.tsv', 'c.tsv', 'stats.tsv', clusters_repr=True, metric='gani', num_alns=4,
                                                                  num_threads=3, verbosity=1, **mins))
        case('stages.deduplicate', lambda: stages.deduplicate(P2, 'o.fna', 'd.txt', prefixes=['a|', 'b|'], gzip_level=6, num_threads=3, verbosity=2))
        case('stages.deduplicate circular', lambda: stages.deduplicate(P2, 'o.fna', 'd.txt', circular=True))
        case('stages.deduplicate circular tr', lambda: stages.deduplicate(P2, 'o.fna', 'd.txt', circular=True, terminal_repeat=10))
        case('stages.deduplicate contained', lambda: stages.deduplicate(P2, 'o.fna', 'd.txt', contained=True, prefixes=['a|', 'b|']))
        case('stages.derep_params', lambda: stages.derep_params(7, 20, 0.5, 30, 0.9, lz, 'cd-hit', 'ani', 5, mins))
        case('stages.derep_params defaults', lambda: stages.derep_params())
        case('stages.dereplicate', lambda: stages.dereplicate(P2, 'c.tsv', False, batch_genomes=7, k=20, kmers_fraction=0.5, min_kmers=30, min_ident=0.9,
                                                              lz=lz, algorithm='cd-hit', metric='ani', num_alns=5, representatives=True, out_table='t.tsv',
                                                              columns=cols, out_repr_fasta='r.fna', num_threads=4, verbosity=2, **mins))
        case('stages.dereplicate defaults', lambda: stages.dereplicate(P2[:1], 'c.tsv', True, tani=0.95))
        case('stages.dereplicate update', lambda: stages.dereplicate(P2[:1], 'c.tsv', True, tani=0.95, db_paths=DB2, prior_path='p.tsv', prior_repr=True))
        # ---- the errors of stages
        case('stages._cluster_params unknown filter', lambda: stages._cluster_params(0, 'tani', 0, False, 0, 0, dict(tani=0.9, cov=0.5)))
        case('stages.cluster unknown filter', lambda: stages.cluster('a', 'i', 'o', tani=0.9, cov=0.5))
        case('stages.cluster mcl keyword', lambda: stages.cluster('a', 'i', 'o', tani=0.9, mcl_prune=0.01, mcl_inflation=2.0))
        case('stages.cluster prior_repr alone', lambda: stages.cluster('a', 'i', 'o', tani=0.9, prior_repr=True))
        case('stages.cluster prior and levels', lambda: stages.cluster('a', 'i', 'o', tani=0.9, prior_path='p', levels=[0.95]))
        case('stages.cluster prior algorithm', lambda: stages.cluster('a', 'i', 'o', tani=0.9, prior_path='p', algorithm='set-cover'))
        case('stages.cluster unknown algorithm', lambda: stages.cluster('a', 'i', 'o', tani=0.9, algorithm='leiden'))
        case('stages.cluster linkage algorithm', lambda: stages.cluster('a', 'i', 'o', tani=0.9, algorithm='cd-hit', out_linkage='l'))
        case('stages.cluster mcl and levels', lambda: stages.cluster('a', 'i', 'o', tani=0.9, algorithm='mcl', levels=[0.95]))
        case('stages.deduplicate circular and contained', lambda: stages.deduplicate(P2, 'o', 'd', circular=True, contained=True))
        case('stages.deduplicate terminal_repeat alone', lambda: stages.deduplicate(P2, 'o', 'd', terminal_repeat=5))
        case('stages.deduplicate contained terminal_repeat', lambda: stages.deduplicate(P2, 'o', 'd', contained=True, terminal_repeat=5))
        case('stages.deduplicate prefixes', lambda: stages.deduplicate(P2, 'o', 'd', prefixes=['a|']))
        case('stages.dereplicate db alone', lambda: stages.dereplicate(P2, 'o', True, tani=0.9, db_paths=DB2))
        case('stages.dereplicate prior alone', lambda: stages.dereplicate(P2, 'o', True, tani=0.9, prior_path='p'))
        case('stages.dereplicate prior_repr alone', lambda: stages.dereplicate(P2, 'o', True, tani=0.9, prior_repr=True))
        case('stages.dereplicate unknown algorithm', lambda: stages.dereplicate(P2, 'o', True, tani=0.9, algorithm='leiden'))
        case('stages.dereplicate unknown filter', lambda: stages.dereplicate(P2, 'o', True, tani=0.9, cov=0.5))
        # ---- api: the library and genome sets
        case('api.version', api.version)
        case('api.device_count', api.device_count)
        case('api.set_device', lambda: api.set_device(2))
        case('GenomeSet.load', lambda: api.GenomeSet.load(P2, False, n_threads=4))
        case('GenomeSet.load_db_new', lambda: api.GenomeSet.load_db_new(DB2, P2[:1], True, n_threads=4))
        codes, offsets = np.array([0, 1, 2, 3, 4, 0, 1], dtype=np.uint8), [0, 4, 7]
        case('GenomeSet.from_codes', lambda: api.GenomeSet.from_codes(codes, offsets, names=['x', 'y']))
        case('GenomeSet.from_codes no names', lambda: api.GenomeSet.from_codes(codes, offsets))
        gs, other = api.GenomeSet(C.c_void_p()), api.GenomeSet(C.c_void_p())
        case('GenomeSet.__len__', lambda: len(gs))
        case('GenomeSet.total_len', lambda: gs.total_len)
        case('GenomeSet.lengths', gs.lengths)
        case('GenomeSet.names', gs.names)
        case('GenomeSet.codes', lambda: gs.codes(1))
        case('GenomeSet.to_device', gs.to_device)
        case('GenomeSet.subset', lambda: gs.subset([2, 0]))
        case('GenomeSet.extend', lambda: gs.extend(other, [1, 2]))
        case('GenomeSet.truncate', lambda: gs.truncate(2))
        case('GenomeSet.reserve', lambda: gs.reserve(1000, 10))
        case('GenomeSet.close', gs.close)
        gs = api.GenomeSet(C.c_void_p())
        case('GenomeSet.dereplicate_set', lambda: gs.dereplicate_set(7, 20, 0.5, 30, 0.9, lz, 'cd-hit', 'ani', 5, **mins))
        case('GenomeSet.dereplicate_set rows', lambda: gs.dereplicate_set(tani=0.95, want_rows=True))
        case('GenomeSet.dereplicate_set prior', lambda: gs.dereplicate_set(tani=0.95, want_rows=True, n_db=2, prior_rep=[0, 0, -1]))
        case('GenomeSet.dereplicate_set n_db', lambda: gs.dereplicate_set(tani=0.95, n_db=2))
        case('GenomeSet.dereplicate_set prior length', lambda: gs.dereplicate_set(tani=0.95, prior_rep=[0, 0]))
        case('GenomeSet.kmer_shared', lambda: gs.kmer_shared(k=20, fraction=0.5, shard=1, n_shards=2, min_shared=3))
        case('GenomeSet.kmer_shared_new', lambda: gs.kmer_shared_new(2, k=20, fraction=0.5, min_shared=3))
        case('GenomeSet.kmer_geometry', lambda: gs.kmer_geometry(k=20, fraction=0.5, shard=1, n_shards=2))
        case('GenomeSet.kmer_set', lambda: gs.kmer_set(1, k=20, fraction=0.5))
        case('GenomeSet.filter_pairs', lambda: gs.filter_pairs([100, 90, 80], pairs, k=20, min_kmers=30, min_ident=0.9))
        case('GenomeSet.write_fltr', lambda: gs.write_fltr('fltr.txt', [100, 90, 80], pairs, k=20, fraction=0.5, min_kmers=30, min_ident=0.9, max_seqs=2))
        case('GenomeSet.align_order', gs.align_order)
        case('GenomeSet.read_filter', lambda: gs.read_filter('fltr.txt', threshold=0.8))
        case('GenomeSet.read_filter none', gs.read_filter)
        case('GenomeSet.align_tasks', lambda: gs.align_tasks(pairs))
        case('GenomeSet.lz_prepare', lambda: gs.lz_prepare(pairs, lz=lz))
        case('GenomeSet.lz_align', lambda: gs.lz_align(tasks, lz=dict(mal=12)))
        case('GenomeSet.lz_align regions', lambda: gs.lz_align(tasks, want_regions=True))
        case('GenomeSet.lz_align empty', lambda: gs.lz_align(tasks[:0]))
        case('GenomeSet.lz_index_dump', lambda: gs.lz_index_dump(1, lz=lz))
        case('GenomeSet.write_ani', lambda: gs.write_ani('ani.tsv', tasks, rows, regions=regions, columns=cols, out_aln='aln.tsv', lz=lz,
                                                         out_filters=dict(ani=0.9, rcov=0.5), num_threads=4))
        case('GenomeSet.write_ani defaults', lambda: gs.write_ani('ani.tsv', tasks, rows))
        # ---- api: clustering on arrays
        case('api.cluster_graph', lambda: api.cluster_graph(3, q, r, w, algorithm='complete'))
        case('api.cluster_graph empty', lambda: api.cluster_graph(0, [], [], []))
        case('api.cluster_graph unknown algorithm', lambda: api.cluster_graph(3, q, r, w, algorithm='average'))
        case('api.cluster_graph lengths', lambda: api.cluster_graph(3, q, r[:2], w))
        case('api.cluster_mcl_graph', lambda: api.cluster_mcl_graph(3, q, r, w, inflation=2.5, prune=1e-3, max_row=64, chaos_eps=1e-2, max_iterations=7))
        case('api.cluster_mcl_graph matrix', lambda: api.cluster_mcl_graph(3, q, r, w, matrix=True))
        case('api.cluster_mcl_graph 2^31', lambda: api.cluster_mcl_graph(big, q, r, w))
        case('api.cluster_mcl_set_table_slots', lambda: api.cluster_mcl_set_table_slots(64))
        case('api.cluster_update_graph', lambda: api.cluster_update_graph(3, q, r, w, [0, -1, -1], algorithm='uclust'))
        case('api.cluster_update_graph 2^31', lambda: api.cluster_update_graph(big, q, r, w, [0, -1]))
        case('api.cluster_update_graph algorithm', lambda: api.cluster_update_graph(3, q, r, w, [0, -1, -1], algorithm='set-cover'))
        case('api.cluster_update_graph prior length', lambda: api.cluster_update_graph(3, q, r, w, [0, -1]))
        case('api.cluster_update', lambda: api.cluster_update('ani.tsv', 'ids.tsv', 'p.tsv', 'c.tsv', algorithm='cd-hit', prior_repr=True, tani=0.9, num_alns=3))
        case('api.cluster_stats_graph', lambda: api.cluster_stats_graph(3, q, r, w, [0, 0, 1]))
        case('api.cluster_stats_graph n_clusters', lambda: api.cluster_stats_graph(3, q, r, w, [0, 0, 1], n_clusters=4))
        case('api.cluster_stats_graph 2^31', lambda: api.cluster_stats_graph(big, q, r, w, [0, 1], n_clusters=big))
        case('api.cluster_stats_graph label length', lambda: api.cluster_stats_graph(3, q, r, w, [0, 0]))
        case('api.cluster_linkage', lambda: api.cluster_linkage(3, q, r, w))
        case('api.cluster_linkage 2^31', lambda: api.cluster_linkage(big, q, r, w))
        case('api.cluster_complete_linkage_graph', lambda: api.cluster_complete_linkage_graph(3, q, r, w))
        case('api.cluster_average_linkage_graph', lambda: api.cluster_average_linkage_graph(3, q, r, w, floor=0.5))
        case('api.cluster_levels', lambda: api.cluster_levels(3, q, r, w, [0.75, 0.85]))
        case('api.cluster_levels 2^31', lambda: api.cluster_levels(big, q, r, w, 0.75))
        case('api.cluster_complete_levels_graph', lambda: api.cluster_complete_levels_graph(3, q, r, w, [0.75]))
        case('api.cluster_average_levels_graph', lambda: api.cluster_average_levels_graph(3, q, r, w, [0.75, 0.85], floor=0.5))
        case('api.cluster_average_similarity', lambda: api.cluster_average_similarity(3 << 32, 4))
        case('api.cluster_average_order_selftest', lambda: api.cluster_average_order_selftest([5, 6, 7], [1, 1, 2], [1, 2, 2], [0, 1, 2], [3, 4, 5], on_device=True))
        case('api.cluster_average_order_selftest lengths', lambda: api.cluster_average_order_selftest([5, 6, 7], [1, 1], [1, 2, 2], [0, 1, 2], [3, 4, 5]))
        # ---- api: deduplicate
        case('api.terminal_repeats', lambda: api.terminal_repeats(seqs, 2))
        case('api.deduplicate', lambda: api.deduplicate(seqs))
        case('api.deduplicate empty', lambda: api.deduplicate([]))
        case('api.deduplicate circular', lambda: api.deduplicate(seqs, circular=True))
        case('api.deduplicate circular tr', lambda: api.deduplicate(seqs, circular=True, terminal_repeat=2))
        case('api.deduplicate contained', lambda: api.deduplicate(seqs, contained=True))
        case('api.deduplicate unknown keyword', lambda: api.deduplicate(seqs, rotate=True, also=1))
        case('api.deduplicate circular and contained', lambda: api.deduplicate(seqs, circular=True, contained=True))
        case('api.deduplicate terminal_repeat alone', lambda: api.deduplicate(seqs, terminal_repeat=2))
        case('api.deduplicate contained terminal_repeat', lambda: api.deduplicate(seqs, contained=True, terminal_repeat=2))
        case('api.deduplicate_files', lambda: api.deduplicate_files(P2, 'o.fna', 'd.txt', circular=True, terminal_repeat=4))
        # ---- api: knobs and measurement
        case('api.dedup_set_hash_bits', lambda: api.dedup_set_hash_bits(64))
        case('api.dedup_set_anchor_symbols', lambda: api.dedup_set_anchor_symbols(8))
        case('api.dedup_set_index_positions', lambda: api.dedup_set_index_positions(1000))
        case('api.set_lz_fit', lambda: api.set_lz_fit(4, 0, 2))
        case('api.set_lz_fit defaults', api.set_lz_fit)
        case('api.set_range_scan', lambda: api.set_range_scan(1))
        case('api.set_placement_trials', lambda: api.set_placement_trials(4))
        case('api.set_new_path', lambda: api.set_new_path(2))
        case('api.kmer_geometry_at', lambda: api.kmer_geometry_at(1 << 20, k=20))
        case('api.rowptr_inline_lo', lambda: api.rowptr_inline_lo(1000, 10))
        case('api.release_device_memory', api.release_device_memory)
        case('api.profile_enable', lambda: api.profile_enable(False))
        case('api.profile_reset', api.profile_reset)
        case('api.profile_get', api.profile_get)
        case('_lib.hip_copy', lambda: _lib.hip_copy(4096, C.c_void_p(8192), 16, to_host=True))
        # ---- distributed: the array-level functions (no process group)
        comm = distributed.Comm(C.c_void_p(), lib)
        case('distributed.prefilter_counts', lambda: distributed.prefilter_counts(gs, comm, 20, 0.5, min_shared=3))
        case('distributed.align_pairs_share', lambda: distributed.align_pairs_share(gs, pairs, 4, 1))
        case('distributed.align_pairs', lambda: distributed.align_pairs(gs, pairs, comm, lz=lz))
        case('distributed.align_rows', lambda: distributed.align_rows(gs, tasks, comm, lz=dict(msl=8), want_regions=True))
        case('distributed.align_rows no regions', lambda: distributed.align_rows(gs, tasks, comm))
        case('distributed.align_owner', lambda: distributed.align_owner(tasks, 3, 4))
        case('distributed.Comm', lambda: [comm.describe(), comm.selftest(64)])
        comm.close()
    return out


def constants():
    dtypes = {name: {'descr': [list(d) for d in getattr(api, name).descr], 'itemsize': getattr(api, name).itemsize}
              for name in ('PAIR_DTYPE', 'TASK_DTYPE', 'STAT_DTYPE', 'REGION_DTYPE', 'LINKAGE_DTYPE', 'AVERAGE_LINKAGE_DTYPE', 'CLUSTER_STAT_DTYPE')}
    return dict(dtypes=dtypes, ALIGN_FIELDS=[list(cli.ALIGN_FIELDS), list(api.ALIGN_FIELDS)], ALIGN_OUTFMT=_plain(cli.ALIGN_OUTFMT),
                DEFAULT_LZ=[dict(stages.DEFAULT_LZ), dict(api.DEFAULT_LZ)], CLUSTER_FILTERS=list(stages.CLUSTER_FILTERS),
                dist_env=list(distributed.dist_env()))


def surface():
    helps, cases, errors = cli_surface()
    return dict(generator='tools/make_python_surface.py', help=helps, cli=cases, cli_errors=errors, c_calls=c_call_surface(),
                constants=constants())


def render(doc):
    """The fixture's text: help texts on lines of their own, every case as one line of compact JSON."""
    parts = []
    for key, value in doc.items():
        if isinstance(value, list):
            body = '[\n' + ',\n'.join(json.dumps(x, separators=(',', ':')) for x in value) + '\n]'
        elif key == 'help':
            body = json.dumps(value, indent=0)
        else:
            body = json.dumps(value, separators=(',', ':'))
        parts.append(f'{json.dumps(key)}: {body}')
    return '{\n' + ',\n'.join(parts) + '\n}\n'


def main():
    text = render(surface())
    FIXTURE.write_text(text)
    doc = json.loads(text)
    print(f'{FIXTURE.relative_to(ROOT)}: {len(text)} bytes, {len(doc["cli"])} command lines, {len(doc["cli_errors"])} usage errors, '
          f'{len(doc["c_calls"])} call cases')


if __name__ == '__main__':
    main()
