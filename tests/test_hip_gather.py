"""wai_gather_rows / wai_gather_fluid (include/waiwera_hip.h) at the ABI: rows that live on two ranks' devices arrive on
the root at their places, bit for bit -- a gather moves data, so nothing here has a tolerance.

The mesh is 4 x 3 x 2 cells, rank 0 owning 17 of them and rank 1 seven; the two ranks share ONE GPU over the loop-back
transport of tests/loopback_rccl (tests/test_hip_multirank.py), so what is checked is the library's protocol -- counts,
slabs, places, the claim array -- and that no rank leaves a collective out, which would end the run at the queue timeout
instead of hanging it.  Nothing is claimed about RCCL between real devices.  The two ranks are started once and walk every
case in one fixed order; the tests read what they sent back.

Without the gather none of this imports: the symbols are missing from the library."""
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

from tests.test_hip_multirank import LOOPBACK, _default_overlap, _own_cus

pytestmark = pytest.mark.gpu
DIMS, BRICK, N = (4, 3, 2), (2, 3, 2), 24
SPLIT = 17                                   # rank 0 owns cells 0 .. 16, rank 1 the other 7
BIG = (10000, 40000)                         # 50 000 rows of 3: rank 1's slab is 1.28 MB, above the transport's 1 MB chunk
FIELDS = [0, 1, 2, 9, 7, 12]                 # columns of the fluid record, not in order


def _places():
    """a non-monotone permutation of the 24 places: rank 0 sends to the first 17 entries, rank 1 to the rest"""
    p = np.random.default_rng(7).permutation(N).astype(np.int32)
    assert (np.diff(p[:SPLIT]) < 0).any() and (np.diff(p[SPLIT:]) < 0).any()
    return p


def _rows(rank, n, ncomp, seed=0):
    return np.random.default_rng(100 * seed + rank).standard_normal((n, ncomp))


def _context(rank, world):
    from waiwera_amd.cases import make_case, scaled
    from waiwera_amd.flow_simulation import FlowSimulation
    from waiwera_amd.partition import partition_mesh
    g, lm, prim, region = make_case(dims=DIMS, brick=BRICK, eos="we")
    gid = np.arange(N)
    if world > 1:
        lm, gid = partition_mesh(lm, (np.arange(N) >= SPLIT).astype(int), rank, chunk=16, world=world)
    sim = FlowSimulation(lm, eos="we", device=0)
    sim.set_regions(region[gid])
    return sim, lm, np.ascontiguousarray(scaled(prim[gid], region[gid]).ravel())


def _cases(sim, lm, y, rank, world):
    """every case, in the one order both ranks walk; -> {case: what the rank got back}"""
    import torch
    from waiwera_amd.lib import WaiError
    place = _places()
    mine = place[:SPLIT] if rank == 0 else place[SPLIT:]
    if world == 1:
        mine = place
    n = mine.size
    res = {}
    for ncomp in (1, 3):                                              # host rows, host out
        res["host%d" % ncomp] = sim.gather_rows(_rows(rank, n, ncomp), mine, N)
    dev = torch.from_numpy(_rows(rank, n, 3, seed=1)).to("cuda:0")   # device rows; the root's out a device tensor too
    out = torch.full((N, 3), float("nan"), dtype=torch.float64, device="cuda:0") if rank == 0 else None
    sim.gather_rows(dev, mine, N, out=out)
    res["device"] = out.cpu().numpy() if rank == 0 else None
    for who in range(world):                                          # no rows on rank `who`: the other's places only
        res["empty%d" % who] = sim.gather_rows(np.zeros((0, 2)) if rank == who else _rows(rank, n, 2, seed=2),
                                               mine[:0] if rank == who else mine, N)
    nb = BIG[rank] if world > 1 else sum(BIG)
    first = 0 if rank == 0 else BIG[0]
    big = np.arange(first, first + nb, dtype=np.float64)[:, None] * 4.0 + np.arange(3)
    res["big"] = sim.gather_rows(big, (sum(BIG) - 1 - np.arange(first, first + nb)).astype(np.int32), sum(BIG))
    # a place claimed twice (by the two ranks; on one rank by two rows), and one out of range: an error on the root that
    # names the place, and the next gather works
    for tag, bad in (("duplicate", int(place[0])), ("range", N + 5)):
        idx = mine.copy()
        if rank == world - 1:
            idx[-1] = bad
        try:
            sim.gather_rows(_rows(rank, n, 2, seed=3), idx, N)
            res[tag] = None
        except WaiError as e:
            res[tag] = str(e)
    res["after"] = sim.gather_rows(_rows(rank, n, 1, seed=4), mine, N)
    # the fluid record's columns, packed on the device, against wai_get_fluid + column selection + wai_gather_rows
    assert sim.pre_eval(0.0, y) == 0
    cells = np.asarray(lm.owned_gid, dtype=np.int32) if world > 1 else np.arange(N, dtype=np.int32)
    a0, e0 = sim.comm_stats()
    g0 = sim.gather_stats()
    res["fluid"] = sim.gather_fluid(FIELDS, cells, N)
    a1, e1 = sim.comm_stats()
    res["calls"] = (a1 - a0, e1 - e0, sim.gather_stats() - g0)
    res["fluid_ref"] = sim.gather_rows(np.ascontiguousarray(sim.fluid()[: lm.n_owned][:, FIELDS]), cells, N)
    res["local"] = {k: _rows(rank, n, c, seed=s) for k, c, s in (("host1", 1, 0), ("host3", 3, 0), ("device", 3, 1),
                                                                  ("empty", 2, 2), ("after", 1, 4))}
    return res


def _worker(rank, world, uid_q, q):
    os.environ["WAI_RCCL_LIB"] = LOOPBACK
    _own_cus(rank, world)
    _default_overlap()
    from waiwera_amd import lib as wl
    if rank == 0:
        uid = wl.comm_unique_id()
        for _ in range(world - 1):
            uid_q.put(uid)
    else:
        uid = uid_q.get(timeout=120)
    before = wl.device_memory()
    sim, lm, y = _context(rank, world)
    sim.comm_init(rank, world, uid)
    res = _cases(sim, lm, y, rank, world)
    sim.destroy()
    res["memory"] = (before, wl.device_memory())
    q.put((rank, res))


@pytest.fixture(scope="module")
def two_ranks():
    assert os.path.exists(LOOPBACK), "build first: python __graft_entry__.py"
    world = 2
    ctx = mp.get_context("spawn")
    q, uid_q = ctx.Queue(), ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, uid_q, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = dict(q.get(timeout=240) for _ in range(world))
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.exitcode is None:
                p.kill()
    assert [p.exitcode for p in procs] == [0] * world
    return res


@pytest.fixture(scope="module")
def one_rank():
    """no communicator at all: the same cases on the test's own process"""
    from waiwera_amd import lib as wl
    before = wl.device_memory()
    sim, lm, y = _context(0, 1)
    res = _cases(sim, lm, y, 0, 1)
    sim.destroy()
    res["memory"] = (before, wl.device_memory())
    return {0: res}


def _expected(res, key, local_key=None, ncomp=None, senders=(0, 1)):
    """what the root must hold: NaN where nobody sent, the concatenated input at its places"""
    place = _places()
    parts = [(place[:SPLIT], 0), (place[SPLIT:], 1)] if len(res) == 2 else [(place, 0)]
    loc = [res[r]["local"][local_key or key] for _, r in parts]
    want = np.full((N, ncomp or loc[0].shape[1]), np.nan)
    for (idx, r), rows in zip(parts, loc):
        if r in senders:
            want[idx] = rows
    return want


@pytest.mark.parametrize("key", ["host1", "host3", "device", "after"])
def test_rows_arrive_at_their_places_bit_for_bit(two_ranks, key):
    """ncomp 1 and 3 from host arrays, 3 from device tensors into a device tensor, and the gather after the two refused
    ones: the root's array is the two ranks' input at the permuted places, every bit; the other rank gets nothing back"""
    assert two_ranks[1][key] is None
    assert np.array_equal(two_ranks[0][key], _expected(two_ranks, key))


@pytest.mark.parametrize("who", [0, 1])
def test_a_rank_without_rows(two_ranks, who):
    """n_local = 0 on the root, and on the other rank: the call succeeds, the sender's rows are in place and the places
    nobody sent still hold the NaN they were filled with"""
    got, want = two_ranks[0]["empty%d" % who], _expected(two_ranks, "empty", ncomp=2, senders=(1 - who,))
    assert np.isnan(want).any(axis=1).sum() == (SPLIT if who == 0 else N - SPLIT)
    assert np.array_equal(got, want, equal_nan=True)


def test_a_message_longer_than_a_transport_chunk(two_ranks):
    """50 000 rows of 3 doubles, 40 000 of them from rank 1: its slab of 4 doubles a row is 1.28 MB and crosses the
    transport's chunk boundary (and the library's own message pieces of 512 KB).  Places run backwards"""
    n = sum(BIG)
    want = (np.arange(n, dtype=np.float64)[:, None] * 4.0 + np.arange(3))[::-1]
    assert BIG[1] * 4 * 8 > 1 << 20
    assert np.array_equal(two_ranks[0]["big"], want)


def test_a_place_claimed_twice_and_one_out_of_range(two_ranks, one_rank):
    """both are errors on the root, whose text names the place and who sent it; the sending rank has done its part and
    returns; nothing hangs, and the next gather is right (test_rows_arrive_at_their_places_bit_for_bit[after])"""
    p0 = int(_places()[0])
    for res, second in ((two_ranks, "rank 1 (its row %d)" % (N - SPLIT - 1)), (one_rank, "rank 0 (its row %d)" % (N - 1))):
        dup, rng = res[0]["duplicate"], res[0]["range"]
        assert dup is not None and "place %d is claimed twice" % p0 in dup and "rank 0 (its row 0)" in dup and second in dup, dup
        assert rng is not None and "place %d sent by %s" % (N + 5, second) in rng and "outside [0, %d)" % N in rng, rng
    assert two_ranks[1]["duplicate"] is None and two_ranks[1]["range"] is None


def test_fluid_columns_packed_on_the_device(two_ranks, one_rank):
    """wai_gather_fluid equals wai_get_fluid, column selection on the host and wai_gather_rows, bit for bit; every cell is
    filled (the record has no NaN) and pressure and temperature are not one column twice"""
    for res in (two_ranks, one_rank):
        got, ref = res[0]["fluid"], res[0]["fluid_ref"]
        assert got.shape == (N, len(FIELDS)) and np.isfinite(got).all()
        assert np.array_equal(got, ref)
        assert not np.array_equal(got[:, 0], got[:, 1])
    # the two ranks together hold the one-rank run's record: the same state, the same kernel
    assert np.array_equal(two_ranks[0]["fluid"], one_rank[0]["fluid"])


def test_one_rank_without_a_communicator(one_rank):
    """world = 1, no wai_comm_init: the call is the permutation copy alone -- host and device rows, a hole left as it was,
    the long case -- and no collective is counted"""
    r = one_rank[0]
    for key in ("host1", "host3", "device", "after"):
        assert np.array_equal(r[key], _expected(one_rank, key))
    assert np.isnan(r["empty0"]).all()                       # the only rank sent nothing: every place is a hole
    n = sum(BIG)
    assert np.array_equal(r["big"], (np.arange(n, dtype=np.float64)[:, None] * 4.0 + np.arange(3))[::-1])
    assert r["calls"] == (0, 0, 0)


def test_both_ranks_make_the_same_collective_calls(two_ranks):
    """one gather call: one all-reduce (the row counts), no neighbour exchange, one gather -- on both ranks alike"""
    assert two_ranks[0]["calls"] == two_ranks[1]["calls"] == (1, 0, 1)


def test_destroy_returns_the_gather_buffers(two_ranks, one_rank):
    """the library's count of live device allocations is back where it was before the context was made, on each rank"""
    for res in (two_ranks, one_rank):
        for rank, r in res.items():
            before, after = r["memory"]
            assert after == before, (rank, before, after)
