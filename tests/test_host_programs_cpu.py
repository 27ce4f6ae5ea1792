"""The library's host code under sanitizers, through stand-alone programs (tests/host_programs/): no GPU, nothing preloaded.

The recipe compiles the host sources for the host and links them with small programs that have their own main, three times:
`plain` (-O1 -g), `asan` (address + undefined behaviour) and `tsan` (thread; the threaded programs only).  Every program
checks its own properties and ends with status 0 only if all held; here each one runs in a child process with a time limit,
must end with status 0 without a sanitizer report on stderr, and the sanitized builds must print what the plain build prints,
byte for byte (every accepted input gives the same bytes, every rejected one the same status and message).

Seconds measured on eight cores for the `asan` runs, which `plain` shares, and for the `tsan` runs (the limit of a
run is ten times its value):

    gunzip_corpus              30 s      (plain 10 s.  With the decoder as it was before the fixes that came with this file the
                                          plain build did not finish in 300 s and the asan build not in 400 s: a cut stream was
                                          decoded on with zeros until a 1 MiB output chunk was full, and a trailer claiming 4 GiB
                                          had them reserved -- and, under asan, their shadow poisoned -- before any byte was verified.  The
                                          reservation is pinned on its own: the program sees every realloc of the decoder and holds the
                                          largest request of each call to 1.5 (1032 n + 2 MiB); the earlier decoder asked for 4.3 GB
                                          for the 41-byte named case, this one for 1.1 MB)
    gunzip_corpus --big         7 s      (tsan 13 s)
    text_readers               11 s
    fasta_ingest               11 s      (tsan, 3 and 16 threads: 13 s; measured again with the directory and database + new
                                          cases in: 10.3 s and 12.3 s, so both values stay)
    writers_and_lists           3 s      (tsan 9 s)

The valid streams that vg_fast_gunzip declines and leaves to zlib are pinned below (FELL_BACK): measured, none -- every class
of the corpus (levels 0-9, fixed, Huffman-only, RLE, two and three members, an empty member, a named header, zero padding) is
taken by the fast path at every length and for every kind of text.
"""
import os
import pathlib
import shutil
import subprocess

import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent
HERE = ROOT / 'tests' / 'host_programs'
BUILD = HERE / '_build'
GOLDEN = ROOT / 'tests' / 'golden' / 'example'

# program: arguments, seconds of the asan run, arguments of the tsan run (None: no tsan build of it), seconds of the tsan run
PROGRAMS = {
    'gunzip_corpus': ([], 30, None, None),
    'gunzip_corpus --big': (['--big'], 7, ['--big'], 13),
    'text_readers': ([str(GOLDEN)], 11, None, None),
    'fasta_ingest': ([str(GOLDEN)], 11, [str(GOLDEN), '3', '16'], 13),
    'writers_and_lists': ([], 3, ['3', '16'], 9),
}
FELL_BACK = set()        # "class kind-length" of the valid streams the fast gunzip leaves to zlib
REPORTS = ('AddressSanitizer', 'runtime error', 'ThreadSanitizer')
ENV = dict(ASAN_OPTIONS='detect_leaks=0:halt_on_error=1:abort_on_error=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1',
           TSAN_OPTIONS='halt_on_error=1:second_deadlock_stack=1')


def _hipcc():
    for cand in (os.environ.get('HIPCC'), shutil.which('hipcc'), '/opt/rocm/bin/hipcc'):
        if cand and pathlib.Path(cand).exists():
            return cand
    return None


@pytest.fixture(scope='module')
def built():
    hipcc = _hipcc()
    if hipcc is None or shutil.which('make') is None:
        pytest.skip('no hipcc or no make: the host programs cannot be built')
    r = subprocess.run(['make', '-C', str(HERE), '-j8', 'all', 'HIPCC=' + hipcc], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-4000:]
    return BUILD


def _run(built, variant, name, args, seconds):
    env = dict(os.environ, **ENV)
    p = subprocess.run([str(built / variant / name.split()[0])] + args, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=10 * seconds)
    tail = (p.stdout[-1500:] + '\n' + p.stderr[-2500:])
    assert p.returncode == 0, (variant, name, p.returncode, tail)
    for word in REPORTS:
        assert word not in p.stderr, (variant, name, tail)
    return p.stdout


@pytest.mark.parametrize('name', list(PROGRAMS))
def test_host_program_plain_and_asan(built, name):
    """status 0, no report, and the asan build prints the plain build's results byte for byte"""
    args, seconds, _, _ = PROGRAMS[name]
    plain = _run(built, 'plain', name, args, seconds)
    asan = _run(built, 'asan', name, args, seconds)
    assert plain.rstrip().endswith('ok') and len(plain.splitlines()) > 5
    assert asan == plain
    if name == 'gunzip_corpus':
        lines = plain.splitlines()
        fell = {l[len('fell back: '):] for l in lines if l.startswith('fell back: ') and not l.endswith('valid streams')}
        assert fell == FELL_BACK
        assert 'fell back: %d valid streams' % len(FELL_BACK) in lines
        assert sum(l.startswith('stream ') for l in lines) == 25 * 18       # 6 lengths x 4 kinds + the empty text, 18 classes each
        assert 'named cases: cut-costs-no-more, isize-4gib' in lines


@pytest.mark.parametrize('name', [n for n in PROGRAMS if PROGRAMS[n][2] is not None])
def test_host_program_tsan(built, name):
    """the threaded paths at 3 and 16 threads (the CRC pieces of a text above 32 MiB, the BGZF ingest, the deduplicate stage's gzip
    writer, the writers and list builders): status 0 and no report"""
    plain_args, plain_seconds, args, seconds = PROGRAMS[name]
    out = _run(built, 'tsan', name, args, seconds)
    assert out.rstrip().endswith('ok')
    if name == 'writers_and_lists':       # the same bytes as the plain build at 1, 3 and 16 threads
        assert out == _run(built, 'plain', name, plain_args, plain_seconds)
