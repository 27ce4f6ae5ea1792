"""bench.py: a plain run adds nothing to the headline step; --full adds the legs beside it, each still skipped by its --no-*
option and by the runs it does not apply to."""
import pytest

import bench

LEGS = ('cli_wall', 'out_aln', 'other_workloads', 'cpu_baseline', 'sha256')


def _legs(argv, world=1):
    args = bench.parse_args(argv)
    return bench.full_legs(args, world, bench.synth.WORKLOADS[args.workload]['kind'])


@pytest.mark.parametrize('argv', [[], ['--gpus', '1', '--steps', '20', '--warmup', '5'], ['--workload', 'phage-1k'],
                                  ['--dump-outputs', 'out', '--cpu-reps', '1']])
def test_plain_run_adds_no_leg(argv):
    assert not any(_legs(argv).values())
    assert not any(_legs(argv, world=2).values())


def test_full_adds_every_leg_of_the_default_set():
    assert _legs(['--full']) == dict.fromkeys(LEGS, True)
    assert _legs(['--full', '--gpus', '1', '--steps', '20', '--warmup', '5']) == dict.fromkeys(LEGS, True)


@pytest.mark.parametrize('flag,leg', [('--no-cpu-baseline', 'cpu_baseline'), ('--no-cli-wall', 'cli_wall'),
                                      ('--no-other-workloads', 'other_workloads'), ('--no-out-aln', 'out_aln')])
def test_no_option_skips_its_leg_only(flag, leg):
    got = _legs(['--full', flag])
    assert got == dict(dict.fromkeys(LEGS, True), **{leg: False})


def test_full_legs_follow_the_run():
    # the other workloads belong to the default set at its size, the CPU baseline to a family set
    assert _legs(['--full', '--workload', 'phage-1k']) == dict(dict.fromkeys(LEGS, True), other_workloads=False)
    assert _legs(['--full', '--count', '500']) == dict(dict.fromkeys(LEGS, True), other_workloads=False)
    assert _legs(['--full', '--workload', 'imgvr-10k']) == dict(dict.fromkeys(LEGS, True), other_workloads=False, cpu_baseline=False)
    # more than one rank: only the set's digest
    assert _legs(['--full'], world=2) == dict(dict.fromkeys(LEGS, False), sha256=True)


def test_argument_errors_stay():
    for argv in (['--steps', '0'], ['--warmup', '-1']):
        with pytest.raises(SystemExit):
            bench.parse_args(argv)
