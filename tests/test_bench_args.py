"""bench.py's command line on the host: a plain run times the steps only, --full opts into the runs of their own, and the
options that skip parts of a --full run still parse."""
import sys

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_a_plain_run_leaves_out_the_extra_runs(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "4", "--warmup", "2")
    assert (a.gpus, a.steps, a.warmup, a.full) == (1, 4, 2, False)


def test_full_keeps_its_skip_options(monkeypatch):
    a = _parse(monkeypatch, "--full", "--no-cpu-baseline", "--no-config4", "--no-probes")
    assert a.full and a.no_cpu_baseline and a.no_config4 and a.no_probes
