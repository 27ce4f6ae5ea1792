"""The row-pointer rule of a prefilter pass, asked on the host (vg_rowptr_inline_lo: the entry calls the function the passes call).
A pass whose genome list holds `entries` slots over n genomes lets a row pointer carry a genome id (value 0xFFFFFFFF - id, so the
values from inline_lo = 2^32 - n on) exactly when the plain values 1 .. entries stay below inline_lo.  No device is needed."""
import os
import subprocess
import sys

import pytest

from vclust_amd import _lib, api


@pytest.mark.parametrize('n_genomes', [1, 2, 100_000, 1 << 20, (1 << 31) + 5])
def test_boundary(n_genomes):
    """entries + n_genomes = 2^32 - 1: on; 2^32 and 2^32 + 1: off"""
    at = (1 << 32) - n_genomes                                   # entries at which the sum is 2^32 = inline_lo itself
    assert api.rowptr_inline_lo(at - 1, n_genomes) == at
    assert api.rowptr_inline_lo(at, n_genomes) == 0
    assert api.rowptr_inline_lo(at + 1, n_genomes) == 0
    assert 0xFFFFFFFF - (n_genomes - 1) == at                    # the value of the largest genome id is inline_lo itself


def test_sizes_of_the_benchmark_and_edges():
    assert api.rowptr_inline_lo(4_096_000_004, 100_000) == (1 << 32) - 100_000      # 100 000 genomes x 40 960 positions + the slack
    assert api.rowptr_inline_lo(0, 1) == (1 << 32) - 1
    assert api.rowptr_inline_lo(0, 0) == 0                       # no genome: nothing to carry
    assert api.rowptr_inline_lo(1 << 32, 1) == 0 and api.rowptr_inline_lo(1 << 40, 5) == 0
    assert api.rowptr_inline_lo(0, 1 << 32) == 0 and api.rowptr_inline_lo(5, 1 << 40) == 0
    for bad in (lambda: api.rowptr_inline_lo(-1, 5), lambda: api.rowptr_inline_lo(5, -1)):
        with pytest.raises(_lib.VclustGpuError) as e:
            bad()
        assert e.value.code == -1


def test_developer_switch_forces_off():
    """VG_ROWPTR_INLINE=0 is read when the library is loaded, beside VG_DEV_SWITCHES=1 only: a fresh process."""
    root = str(_lib.PKG_DIR.parent)
    code = "import sys; sys.path.insert(0, %r); from vclust_amd import api; print(api.rowptr_inline_lo(1000, 10))" % root

    def run(**env):
        return subprocess.run([sys.executable, '-c', code], env={**os.environ, **env}, stdout=subprocess.PIPE, text=True, check=True).stdout.split()
    assert run() == [str((1 << 32) - 10)]
    assert run(VG_DEV_SWITCHES='1', VG_ROWPTR_INLINE='0') == ['0']
    assert run(VG_DEV_SWITCHES='1', VG_ROWPTR_INLINE='1') == [str((1 << 32) - 10)]
    assert run(VG_ROWPTR_INLINE='0') == [str((1 << 32) - 10)]                    # not a developer run: ignored
