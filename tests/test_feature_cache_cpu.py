"""CPU: pipeline.plan_misses, the host-side planner of the resident trainer's feature cache --
which positions of an epoch's row order each step has to compute, given what is already cached."""
import numpy as np

from abd_amd import parallel_dp as DP
from abd_amd.pipeline import plan_misses


def bounds(n, batch, rank=0, world=1):
    """(start, end) of this rank's shard of every global batch of an n-row epoch (drop_last=False)."""
    out, pos = [], 0
    while pos < n:
        g = min(batch * world, n - pos)
        out.append(DP.shard_range(pos, g, rank, world))
        pos += g
    return out


def test_all_miss_all_hit_and_mixed():
    rows = np.array([5, 2, 7, 0, 3, 6, 1, 4])
    cached = np.zeros(8, bool)
    plan = plan_misses(rows, cached, bounds(8, 4))
    assert [p.tolist() for p in plan] == [[0, 1, 2, 3], [4, 5, 6, 7]]          # positions in the epoch order
    assert not cached.any()                                                    # the planner only reads `cached`
    cached[:] = True
    assert [p.tolist() for p in plan_misses(rows, cached, bounds(8, 4))] == [[], []]
    cached[:] = False
    cached[[2, 0, 6]] = True                                                   # rows, not positions
    plan = plan_misses(rows, cached, bounds(8, 4))
    assert [rows[p].tolist() for p in plan] == [[5, 7], [3, 1, 4]]
    assert [p.tolist() for p in plan] == [[0, 2], [4, 6, 7]]
    assert all(p.dtype == np.int64 for p in plan)


def test_short_tail_batch():
    rows = np.array([3, 9, 1, 0, 8, 2, 6, 11, 4, 10, 7, 5])
    cached = np.zeros(12, bool)
    cached[[7, 0]] = True
    b = bounds(12, 5)
    assert b == [(0, 5), (5, 10), (10, 12)]
    plan = plan_misses(rows, cached, b)
    assert [p.tolist() for p in plan] == [[0, 1, 2, 4], [5, 6, 7, 8, 9], [11]]


def test_world_two_shards_only_this_ranks_rows():
    rows = np.arange(10)[::-1].copy()
    for rank in (0, 1):
        b = bounds(10, 2, rank, 2)          # global batches of 4, 4 and a tail of 2
        plan = plan_misses(rows, np.zeros(10, bool), b)
        assert [p.tolist() for p in plan] == [list(range(s, e)) for s, e in b]
        assert sum(e - s for s, e in b) == 5
    b0, b1 = bounds(10, 2, 0, 2), bounds(10, 2, 1, 2)
    both = sorted(p for s, e in b0 + b1 for p in range(s, e))
    assert both == list(range(10))          # the two ranks' shards tile the epoch
    # a tail with fewer rows than ranks leaves one rank an empty shard: an empty plan for that step
    b = bounds(9, 2, 1, 2)
    assert b[-1][0] == b[-1][1]
    assert plan_misses(np.arange(9), np.zeros(9, bool), b)[-1].size == 0


def test_row_planned_once_within_and_across_epochs():
    cached = np.zeros(6, bool)
    # not a permutation: row 4 shows up in steps 0 and 1, row 2 twice inside step 1
    rows = np.array([4, 1, 0, 4, 2, 2])
    plan = plan_misses(rows, cached, [(0, 3), (3, 6)])
    assert [p.tolist() for p in plan] == [[0, 1, 2], [4]]
    planned = np.concatenate([rows[p] for p in plan])
    assert len(planned) == len(set(planned.tolist()))
    # two epochs of a 12-row table: epoch 2 sees another order and other batch contents, no misses
    rng = np.random.default_rng(0)
    cached = np.zeros(12, bool)
    e1, e2 = rng.permutation(12), rng.permutation(12)
    p1 = plan_misses(e1, cached, bounds(12, 5))
    assert sum(p.size for p in p1) == 12
    for p in p1:                             # what the trainer does after each step's launch
        cached[e1[p]] = True
    assert sum(p.size for p in plan_misses(e2, cached, bounds(12, 5))) == 0
    # an epoch cut short after its first step: only that step's rows count as cached afterwards
    cached[:] = False
    cached[e1[p1[0]]] = True
    p2 = plan_misses(e2, cached, bounds(12, 5))
    assert sorted(np.concatenate([e2[p] for p in p2]).tolist()) == sorted(set(range(12)) - set(e1[:5].tolist()))
