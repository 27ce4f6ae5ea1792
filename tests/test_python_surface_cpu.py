"""The Python front end's recorded surface (tests/golden/python_surface.json, written by tools/make_python_surface.py): help texts,
the stage calls and log lines of a list of command lines, every usage error, the arguments of every C call behind stages, api and
distributed, the values they return and the errors they raise, and the record dtypes.  Recomputed here and compared for equality; no
device and no built library are needed."""
import json
import pathlib
import subprocess
import sys

import pytest

from tools import make_python_surface as mps

ROOT = pathlib.Path(__file__).resolve().parent.parent


@pytest.fixture(scope='module')
def recorded():
    return json.loads(mps.FIXTURE.read_text())


@pytest.fixture(scope='module')
def computed():
    return mps.surface()


def _by_key(items, key):
    return {json.dumps(x[key]) + json.dumps(x.get('env')): x for x in items}


def test_help_texts(recorded, computed):
    assert sorted(computed['help']) == sorted(('vclust',) + mps.SUBCOMMANDS)
    for name, text in recorded['help'].items():
        assert computed['help'][name] == text, name


@pytest.mark.parametrize('section, key', [('cli', 'argv'), ('cli_errors', 'argv'), ('c_calls', 'case')])
def test_cases(recorded, computed, section, key):
    want, got = _by_key(recorded[section], key), _by_key(json.loads(json.dumps(computed[section])), key)
    assert list(got) == list(want)
    for name, case in want.items():
        assert got[name] == case, name


def test_every_usage_error_exits_with_status_2(recorded):
    for case in recorded['cli_errors']:
        assert case['exit'] == 2 and ': error: ' in case['stderr'] and not case['calls'], case['argv']


def test_constants_and_dtypes(recorded, computed):
    assert json.loads(json.dumps(computed['constants'])) == recorded['constants']


def test_fixture_bytes(computed):
    assert mps.render(computed) == mps.FIXTURE.read_text()


def test_the_command_line_imports_neither_numpy_nor_torch():
    code = "import sys, vclust_amd.cli, vclust_amd.stages; assert 'numpy' not in sys.modules and 'torch' not in sys.modules"
    subprocess.run([sys.executable, '-c', code], cwd=ROOT, check=True)
