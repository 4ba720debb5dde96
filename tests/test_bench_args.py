"""CPU: which measurements beside the headline a bench.py run makes.  A plain
run makes none of them; --full makes all; an option given on the command
line wins either way."""
import pytest

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)


def _resolved(argv, dense=False):
    import bench
    a = bench.resolve_extras(bench.parse_args(argv), dense)
    return (a.repeat, a.live_traffic, a.cpu_baseline_iters, a.multi_chain)


@pytest.mark.parametrize("dense", [False, True])
def test_plain_run_makes_no_extra_measurement(dense):
    assert _resolved(["--gpus", "1", "--steps", "20", "--warmup", "5"],
                     dense) == (1, 0, 0, [])


def test_full_restores_every_extra():
    assert _resolved(["--full"]) == (5, 1, 5, [2, 4])
    assert _resolved(["--full"], dense=True) == (5, 1, 2, [4, 8, 16, 32])


def test_explicit_options_win_over_the_default_of_either_mode():
    assert _resolved(["--repeat", "3", "--multi-chain", "4",
                      "--cpu-baseline-iters", "2", "--live-traffic", "1"]) \
        == (3, 1, 2, [4])
    assert _resolved(["--full", "--repeat", "1", "--multi-chain", "0",
                      "--cpu-baseline-iters", "0", "--live-traffic", "0"]) \
        == (1, 0, 0, [])
