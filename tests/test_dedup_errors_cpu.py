"""The argument errors of the five array-level deduplicate calls without a GPU: code and full text of vg_last_error() for a
negative count, decreasing offsets, a null offset array, a missing output / repeat array, min_repeat == 0 and a byte outside
the alphabet.  Every check runs before anything is uploaded.  The texts are the ones the library gave before the checks were
brought together in one place: vg_dedup_seqs names itself whatever the entry point, vg_dedup_terminal_repeats names itself."""
import ctypes as C

import numpy as np
import pytest

from vclust_amd import _lib

EINVAL = -1
SEQ = b'ACGTACJT'                       # two records of four symbols; the second holds a 'J'
OFFSETS = (0, 4, 8)


def arrays(n=2):
    return dict(representative=np.zeros(n, np.int32), strand=np.zeros(n, np.int8), offset=np.zeros(n, np.int64), repeat=np.zeros(n, np.int64))


def ptr(a, ctype):
    return None if a is None else a.ctypes.data_as(C.POINTER(ctype))


def call(entry, ascii=b'ACGTACGT', offsets=OFFSETS, n=2, min_repeat=3, **absent):
    """Runs the entry point on n records; absent: names of output arrays to pass as NULL.  -> (code, vg_last_error())"""
    lib = _lib.load()
    a = arrays()
    a.update({k: None for k in absent})
    off = None if offsets is None else np.asarray(offsets, dtype=np.int64)
    rep, strand, offset, repeat = ptr(a['representative'], C.c_int32), ptr(a['strand'], C.c_int8), ptr(a['offset'], C.c_int64), ptr(a['repeat'], C.c_int64)
    o = ptr(off, C.c_int64)
    if entry == 'vg_dedup_seqs':
        rc = lib.vg_dedup_seqs(ascii, o, n, rep, strand, None)
    elif entry == 'vg_dedup_seqs_ex':
        rc = lib.vg_dedup_seqs_ex(ascii, o, n, C.byref(_lib.DedupOptions(circular=1)), rep, strand, offset, None)
    elif entry == 'vg_dedup_seqs_contained':
        rc = lib.vg_dedup_seqs_contained(ascii, o, n, rep, strand, offset, None, None)
    elif entry == 'vg_dedup_seqs_circular_tr':
        rc = lib.vg_dedup_seqs_circular_tr(ascii, o, n, min_repeat, rep, strand, offset, repeat, None, None)
    else:
        assert entry == 'vg_dedup_terminal_repeats'
        rc = lib.vg_dedup_terminal_repeats(ascii, o, n, min_repeat, repeat)
    return rc, lib.vg_last_error().decode()


SEQS_ENTRIES = ['vg_dedup_seqs', 'vg_dedup_seqs_ex', 'vg_dedup_seqs_contained', 'vg_dedup_seqs_circular_tr']
ENTRIES = SEQS_ENTRIES + ['vg_dedup_terminal_repeats']


def named(entry):
    return 'vg_dedup_terminal_repeats' if entry == 'vg_dedup_terminal_repeats' else 'vg_dedup_seqs'


@pytest.mark.parametrize('entry', ENTRIES)
def test_negative_count(entry):
    assert call(entry, n=-1) == (EINVAL, f'{named(entry)}: negative count')
    assert call(entry, n=-1, offsets=None, representative=1, strand=1, offset=1, repeat=1) == (EINVAL, f'{named(entry)}: negative count')


@pytest.mark.parametrize('entry', ENTRIES)
def test_decreasing_offsets(entry):
    assert call(entry, offsets=(0, 6, 4)) == (EINVAL, f'{named(entry)}: offsets must not decrease')


@pytest.mark.parametrize('entry', ENTRIES)
def test_null_offset_array(entry):
    assert call(entry, offsets=None) == (EINVAL, f'{named(entry)}: null argument')


@pytest.mark.parametrize('entry', ENTRIES)
def test_null_sequence_buffer(entry):
    assert call(entry, ascii=None) == (EINVAL, f'{named(entry)}: null sequence buffer')


def test_null_repeat_array():
    assert call('vg_dedup_seqs_circular_tr', repeat=1) == (EINVAL, 'vg_dedup_seqs_circular_tr: the repeat array is required')
    assert call('vg_dedup_terminal_repeats', repeat=1) == (EINVAL, 'vg_dedup_terminal_repeats: null argument')


def test_null_output_arrays():
    """the three checks of the modes come first, then the shared ones"""
    assert call('vg_dedup_seqs_ex', offset=1) == (EINVAL, 'vg_dedup_seqs_ex: circular mode needs the offset array')
    assert call('vg_dedup_seqs_circular_tr', offset=1) == (EINVAL, 'vg_dedup_seqs_ex: circular mode needs the offset array')
    assert call('vg_dedup_seqs_contained', offset=1) == (EINVAL, 'vg_dedup_seqs_contained: the offset array is required')
    assert call('vg_dedup_seqs_circular_tr', offset=1, repeat=1, offsets=None) == (EINVAL, 'vg_dedup_seqs_circular_tr: the repeat array is required')
    assert call('vg_dedup_seqs_contained', offset=1, offsets=(0, 6, 4)) == (EINVAL, 'vg_dedup_seqs_contained: the offset array is required')
    for entry in SEQS_ENTRIES:
        assert call(entry, representative=1) == (EINVAL, 'vg_dedup_seqs: null argument')
        assert call(entry, strand=1, offsets=(0, 6, 4)) == (EINVAL, 'vg_dedup_seqs: null argument')
    # with nothing to do the arrays are not looked at
    for entry in ENTRIES:
        assert call(entry, n=0, offsets=None, representative=1, strand=1, offset=1, repeat=1)[0] == 0


def test_min_repeat_zero():
    for m in (0, -2):
        assert call('vg_dedup_seqs_circular_tr', min_repeat=m) == (EINVAL, 'vg_dedup_seqs_circular_tr: min_repeat must be at least 1')
        assert call('vg_dedup_terminal_repeats', min_repeat=m) == (EINVAL, 'vg_dedup_terminal_repeats: min_repeat must be at least 1')
    # it is the first check of both
    assert call('vg_dedup_seqs_circular_tr', min_repeat=0, n=-1, repeat=1) == (EINVAL, 'vg_dedup_seqs_circular_tr: min_repeat must be at least 1')
    assert call('vg_dedup_terminal_repeats', min_repeat=0, n=-1, repeat=1) == (EINVAL, 'vg_dedup_terminal_repeats: min_repeat must be at least 1')


@pytest.mark.parametrize('entry', ENTRIES)
def test_byte_outside_the_alphabet(entry):
    assert call(entry, ascii=SEQ) == (EINVAL, "record 1: 'J' is not an IUPAC nucleotide code")
    assert call(entry, ascii=b'AC\x01TACJT') == (EINVAL, "record 0: '\\x01' is not an IUPAC nucleotide code")
