"""rank_launch.run_ranks itself, which every partition test relies on: results in rank order, one failing rank ends the others, and the
deadline ends a rank that never returns.  No process group and no device: the workers save a value, raise, or sleep."""
import multiprocessing
import os
import time

import pytest
import torch

from rank_launch import run_ranks


def saves(rank, world, port, case, out_dir):
    torch.save({"rank": rank, "world": world, "value": torch.load(case)["base"] + rank}, os.path.join(out_dir, f"rank{rank}.pt"))


def rank_one_raises(rank, world, port, case, out_dir):
    if rank == 1:
        raise RuntimeError("rank 1 gives up")
    time.sleep(30)


def sleeps(rank, world, port, case, out_dir):
    time.sleep(30)


def _no_child_alive():
    return not any(p.is_alive() for p in multiprocessing.active_children())


def test_results_come_back_in_rank_order(tmp_path):
    outs = run_ranks(saves, 2, {"base": 40}, tmp_path / "ranks", 60)     # (a directory that does not exist yet)
    assert outs == [{"rank": 0, "world": 2, "value": 40}, {"rank": 1, "world": 2, "value": 41}]
    assert _no_child_alive()


def test_a_failing_rank_ends_the_others_at_once(tmp_path):
    t0 = time.monotonic()
    with pytest.raises(Exception, match="rank 1 gives up"):
        run_ranks(rank_one_raises, 2, {}, tmp_path, 10)
    assert time.monotonic() - t0 < 10
    assert _no_child_alive()


def test_the_deadline_ends_a_rank_that_never_returns(tmp_path):
    t0 = time.monotonic()
    with pytest.raises(TimeoutError, match="world 1 was still running after 2 s"):
        run_ranks(sleeps, 1, {}, tmp_path, 2)
    assert time.monotonic() - t0 < 10
    assert _no_child_alive()
