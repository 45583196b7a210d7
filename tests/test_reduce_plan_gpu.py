"""The reduce's plan (csrc/abi.hip: ReducePlan, reduce_plan): which of the two level loops a call takes.

The level schedule (OTTOHIP_REDUCE_SCHED=1) is written without the split pipelining and the LDS leaf, so either of
those switches selects the loop of blocking reads although the schedule was asked for. The debug listing tells the
loops apart: only the level schedule's level lines carry an "overflow" field (tests/test_reduce_sched_gpu.py).
The pipelined split itself is opt-in (OTTOHIP_SPLIT_PIPE=1, every split of >= OTTOHIP_SPLIT_PIPE_MIN chunks) and
excludes the debug listing; with the schedule asked for beside it, the pipelined loop of blocking reads still runs
and equals the oracle."""
import pytest

import test_covis_gpu as base
import test_reduce_sched_gpu as sched

pytestmark = pytest.mark.gpu


def _blocking_loop_ran(monkeypatch, capfd):
    monkeypatch.setenv("OTTOHIP_REDUCE_SCHED", "1")
    monkeypatch.setenv("OTTOHIP_DEBUG", "1")
    ev, fb, ref = sched._hubs(3)
    capfd.readouterr()
    sched._build_and_check(ev, fb, ref, sched.HUB_ITEMS).free()
    lv = sched._levels(capfd.readouterr().err)
    assert lv, "no level line in the debug listing"
    assert all(v[2] is None for v in lv.values()), lv  # no "overflow" field: the loop of blocking reads


def test_sched_with_split_pipe_takes_blocking_loop(gpu, monkeypatch, capfd):
    monkeypatch.setenv("OTTOHIP_SPLIT_PIPE", "1")
    _blocking_loop_ran(monkeypatch, capfd)


def test_sched_with_lds_leaf_takes_blocking_loop(gpu, monkeypatch, capfd):
    monkeypatch.setenv("OTTOHIP_LDS_LEAF", "1")
    _blocking_loop_ran(monkeypatch, capfd)


def test_sched_with_split_pipe_runs_pipelined(gpu, monkeypatch):
    """No debug listing, so the splits of >= 2 chunks are pipelined (the counter snapshot of the first half)."""
    monkeypatch.setenv("OTTOHIP_REDUCE_SCHED", "1")
    monkeypatch.setenv("OTTOHIP_SPLIT_PIPE", "1")
    monkeypatch.setenv("OTTOHIP_SPLIT_PIPE_MIN", "2")
    monkeypatch.delenv("OTTOHIP_DEBUG", raising=False)
    base.test_heavy_rows_split_and_hash_paths(gpu)
