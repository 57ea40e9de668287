"""World-size-2 gloo test of the sharding + image-plane exchange (CPU)."""

import os
import socket
import traceback

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from optiland_amd.distributed import shard_bounds


def test_shard_bounds_cover_exactly():
    for n in (0, 1, 7, 8, 9, 1000, 10**7 + 3):
        for w in (1, 2, 3, 8):
            b = [shard_bounds(n, w, r) for r in range(w)]
            assert b[0][0] == 0 and b[-1][1] == n
            assert all(b[i][1] == b[i + 1][0] for i in range(w - 1))
            sizes = [hi - lo for lo, hi in b]
            assert max(sizes) - min(sizes) <= 1


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import optiland_amd.tracer as tr
        from optiland_amd.distributed import ShardedTracer
        from tests._fake_engine import OracleEngine
        from tests._util import load_case
        tr._make_engine = lambda table, device: OracleEngine(table, device)
        table, data = load_case("double_gauss_multifield")
        n = 899  # ragged on purpose
        args = [data[k][:n] for k in ("Hx", "Hy", "Px", "Py")]
        t = tr.HipRayTracer(table, dtype=torch.float64)
        st = ShardedTracer(t)
        g = st.trace_generic(*args, 0.4861, exchange="gather")
        r = st.trace_generic(*args, 0.4861, exchange="reduce")
        # fused spot of one field over the global pupil list (7 doubles all-reduced)
        fs = st.trace_spot(0.0, 0.7, data["Px"][:n], data["Py"][:n], 0.4861, center=(0.0, 17.0))
        q.put((rank, g["lo"], g["hi"], g["rays"].x.numpy(), [h.numpy() for h in g["hits"]],
               r["spot"], fs))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_two_rank_shards_equal_single_process():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = sorted([q.get(timeout=150) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(30)
        assert p.exitcode == 0

    # single-process result on the same inputs
    import optiland_amd.tracer as tr
    from tests._fake_engine import OracleEngine
    from tests._util import load_case
    table, data = load_case("double_gauss_multifield")
    n = 899
    eng = OracleEngine(table)
    t = tr.HipRayTracer(table, dtype=torch.float64, engine=eng)
    full = t.trace_generic(*[data[k][:n] for k in ("Hx", "Hy", "Px", "Py")], 0.4861)
    fx, fy, fi = full.x.numpy(), full.y.numpy(), full.i.numpy()

    # shards tile the input order and concatenate to the single-device result, bit for bit
    assert results[0][1] == 0 and results[0][2] == results[1][1] and results[1][2] == n
    cat = np.concatenate([results[0][3], results[1][3]])
    assert np.array_equal(cat, fx)
    # every rank's all-gather output equals the single-device image-plane arrays
    for _, _, _, _, hits, _, _ in results:
        assert np.array_equal(hits[0], fx) and np.array_equal(hits[1], fy)
        assert np.array_equal(hits[2], fi)
    # reduced spot statistics agree with the definition on the full set
    m = fi > 0
    cx, cy = fx[m].mean(), fy[m].mean()
    rms = np.sqrt(np.mean((fx[m] - cx) ** 2 + (fy[m] - cy) ** 2))
    geo = np.sqrt(np.max((fx[m] - cx) ** 2 + (fy[m] - cy) ** 2))
    # sharded fused spot == single-process definition about the same centre
    one = t.trace_generic(0.0, 0.7, data["Px"][:n], data["Py"][:n], 0.4861)
    ox, oy, oi = one.x.numpy(), one.y.numpy(), one.i.numpy()
    om = oi > 0
    for res in results:
        fs = res[6]
        assert fs["count"] == om.sum()
        np.testing.assert_allclose(fs["centroid"], (ox[om].mean(), oy[om].mean()), rtol=1e-12,
                                   atol=1e-13)
        np.testing.assert_allclose(
            fs["rms_radius"], np.sqrt(np.mean(ox[om] ** 2 + (oy[om] - 17.0) ** 2)), rtol=1e-12)
        np.testing.assert_allclose(
            fs["geometric_radius"], np.sqrt(np.max(ox[om] ** 2 + (oy[om] - 17.0) ** 2)),
            rtol=1e-12)
    for _, _, _, _, _, spot, _ in results:
        assert spot["count"] == m.sum()
        np.testing.assert_allclose(spot["centroid"], (cx, cy), rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(spot["rms_radius"], rms, rtol=1e-6)
        np.testing.assert_allclose(spot["geometric_radius"], geo, rtol=1e-10)


def _edge_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import optiland_amd.tracer as tr
        from optiland_amd.distributed import ShardedTracer, spot_statistics
        from tests._fake_engine import OracleEngine
        from tests._util import load_case
        tr._make_engine = lambda table, device: OracleEngine(table, device)
        table, data = load_case("double_gauss_multifield")
        t = tr.HipRayTracer(table, dtype=torch.float64)
        st = ShardedTracer(t)
        # ONE ray over two ranks: rank 1's shard is empty (used to launch a
        # zero-length trace and disagree on n)
        one = [data[k][:1] for k in ("Hx", "Hy", "Px", "Py")]
        r = st.trace_generic(*one, 0.4861, exchange="reduce")
        g = st.trace_generic(*one, 0.4861, exchange="gather")
        # scalar field broadcast over a 3-ray pupil list
        b = st.trace_generic(0.0, 0.7, data["Px"][:3], data["Py"][:3], 0.4861, exchange="gather")
        # nothing reaches the image plane anywhere: NaN statistics, no ZeroDivisionError
        z = torch.zeros(4, dtype=torch.float64)
        dead = spot_statistics(t.engine, z, z, z)
        q.put((rank, r["lo"], r["hi"], r["rays"] is None, r["spot"], g["hits"][0].numpy(),
               b["hits"][0].numpy(), b["n_total"], dead))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_empty_shards_and_dead_bundles():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_edge_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = sorted([q.get(timeout=150) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(30)
        assert p.exitcode == 0
    assert (results[0][1], results[0][2], results[0][3]) == (0, 1, False)
    assert (results[1][1], results[1][2], results[1][3]) == (1, 1, True)
    for res in results:
        assert res[4]["count"] == 1.0 and np.isfinite(res[4]["rms_radius"])
        assert res[5].shape == (1,) and res[6].shape == (3,) and res[7] == 3
        assert res[8]["count"] == 0.0 and np.isnan(res[8]["rms_radius"])
        assert np.isnan(res[8]["geometric_radius"])
    assert np.array_equal(results[0][5], results[1][5])
    assert np.array_equal(results[0][6], results[1][6])


def _field_worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import optiland_amd.tracer as tr
        from optiland_amd import load_system
        from optiland_amd.distributed import ShardedTracer
        from tests import _hostmath as hm
        cls = hm.make_engine_class()
        tr._make_engine = lambda table, device: cls(table, device)
        table = load_system("double_gauss")
        g = np.random.default_rng(5)
        n = 1001  # ragged on purpose
        r, th = np.sqrt(g.random(n)), 2 * np.pi * g.random(n)
        px, py = r * np.cos(th), r * np.sin(th)
        t = tr.HipRayTracer(table, dtype=torch.float64)
        st = ShardedTracer(t)
        block = st.alloc_field_record(n)  # the step loop's form: one block, reused
        first = st.trace_field(0.0, 0.7, px, py, 0.5876, center=(0.0, 15.0), record=block)
        out = st.trace_field(0.0, 0.7, px, py, 0.5876, center=(0.0, 15.0), record=block)
        assert out["result"].record.data_ptr() == block.data_ptr() == \
            first["result"].record.data_ptr()
        fresh = st.trace_field(0.0, 0.7, px, py, 0.5876, center=(0.0, 15.0))
        res = out["result"]
        # the launch writes the first res.n columns of every row; the columns past them are
        # stride padding that no launch touches (whatever the allocator left there)
        assert fresh["result"].n == res.n == out["hi"] - out["lo"]
        assert torch.equal(fresh["result"].record[:, :, : res.n].nan_to_num(),
                           block[:, :, : res.n].nan_to_num())
        q.put((rank, out["lo"], out["hi"], res.record[:, :, : res.n].numpy(), out["spot"]))
    except BaseException:
        q.put((rank, traceback.format_exc()))  # to the parent at once, not after its timeout
        raise
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_two_rank_one_launch_field_step_equals_single_process():
    """`ShardedTracer.trace_field`: generate + trace + record + reduce in ONE launch per rank
    (`ol_trace_generate` with the spot epilogue, ABI 8 -- the per-step form of config C3),
    the 4 KB slot block the only exchange.  The product's engine class on the host build of
    the kernel source, world size 2 over gloo: the shards' records concatenate to the
    single-process record bit for bit and every rank holds the whole-job statistics."""
    from tests import _hostmath as hm
    if not hm.available():
        pytest.skip("hipcc (used as host C++ compiler) missing")
    hm.make_engine_class()  # build before the workers race for it
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_field_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = sorted([q.get(timeout=150) for _ in range(world)], key=lambda t: t[0])
    for res in results:
        assert len(res) == 5, f"rank {res[0]} failed:\n{res[1]}"
    for p in procs:
        p.join(30)
        assert p.exitcode == 0

    import optiland_amd.tracer as tr
    from optiland_amd import load_system
    table = load_system("double_gauss")
    g = np.random.default_rng(5)
    n = 1001
    r, th = np.sqrt(g.random(n)), 2 * np.pi * g.random(n)
    px, py = torch.tensor(r * np.cos(th)), torch.tensor(r * np.sin(th))
    eng = hm.make_engine_class()(table)
    try:
        full = eng.trace_generate(px, py, table.wavelength_index(0.5876), field=(0.0, 0.7))
        rec = full.record[:, :, :n].numpy()
    finally:
        eng.close()
    assert results[0][1] == 0 and results[0][2] == results[1][1] and results[1][2] == n
    cat = np.concatenate([results[0][3], results[1][3]], axis=2)
    assert np.array_equal(cat, rec, equal_nan=True)
    x, y, i = rec[-1, 0], rec[-1, 1], rec[-1, 6]
    m = i > 0
    for res in results:
        s = res[4]
        assert s["count"] == m.sum()
        np.testing.assert_allclose(s["centroid"], (x[m].mean(), y[m].mean()), rtol=1e-12,
                                   atol=1e-13)
        np.testing.assert_allclose(s["rms_radius"],
                                   np.sqrt(np.mean(x[m] ** 2 + (y[m] - 15.0) ** 2)), rtol=1e-12)
        np.testing.assert_allclose(s["geometric_radius"],
                                   np.sqrt(np.max(x[m] ** 2 + (y[m] - 15.0) ** 2)), rtol=1e-12)
    assert results[0][4] == results[1][4]


def _ref_newton_table():
    """The packaged Zernike freeform with the reference's batch-global Newton stop rule switched
    on and a loose tolerance, so that the number of updates depends on the rays of the batch."""
    from optiland_amd import load_system
    from optiland_amd.system import SURF_REFERENCE_NEWTON, GEOM_PLANE, GEOM_STANDARD
    table = load_system("zernike_fresnel_fringe")
    s = table.surfaces
    newton = (s["geom_kind"] != GEOM_PLANE) & (s["geom_kind"] != GEOM_STANDARD)
    assert newton.any()
    s["flags"][newton] |= SURF_REFERENCE_NEWTON
    s["tol"][newton] = 3e-4
    table.__dict__.pop("_ref_newton", None)
    assert table.reference_newton_surfaces()
    return table


def _ref_newton_rays(n):
    """(Hx, Hy, Px, Py): near-axis rays first, the edge of the pupil at the edge of the field
    last -- the first shard alone stops one update earlier than the whole batch."""
    k = np.arange(n)
    th = np.linspace(0.0, 2 * np.pi, n)
    r = np.where(k < n // 2, 0.02, 0.95)
    return np.zeros(n), np.where(k < n // 2, 0.0, 1.0), r * np.cos(th), r * np.sin(th)


def _newton_worker(rank, world, port, q, n):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import optiland_amd.tracer as tr
        from optiland_amd.distributed import ShardedTracer
        from tests import _hostmath as hm
        cls = hm.make_engine_class()
        tr._make_engine = lambda table, device: cls(table, device)
        table = _ref_newton_table()
        t = tr.HipRayTracer(table, dtype=torch.float64)
        st = ShardedTracer(t)
        wl = float(table.wavelengths[0])
        out = st.trace_generic(*_ref_newton_rays(n), wl, exchange="reduce")
        # (the exchange is installed for the sharded call only: a trace this rank makes by
        # itself afterwards must not wait for the other ranks)
        assert t.engine.newton_count_hook is None
        if rank == 0:
            t.trace_generic(*[a[:8] for a in _ref_newton_rays(max(n, 8))], wl)
        rays = out["rays"]
        got = None if rays is None else np.stack([np.asarray(getattr(rays, k))
                                                  for k in ("x", "y", "z", "L", "M", "N", "opd")])
        q.put((rank, out["lo"], out["hi"], got, out["spot"]))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(240)
@pytest.mark.parametrize("n", [400, 1])
def test_reference_newton_counts_are_those_of_the_whole_batch_when_sharded(n):
    """`reference_newton`: the reference's Newton loop makes the same number of updates for
    every ray of a trace call (newton_raphson.py:137-166), so a batch sharded over ranks has to
    take the maximum over its shards (`HipSystem.newton_count_hook`, one 8 S-byte MAX all-reduce
    per counting launch).  World size 2 over gloo on the host build of the kernel source: the
    shards concatenate to the single-process trace bit for bit -- the paraxial shard alone would
    have stopped earlier -- and a rank without rays (n = 1) takes part in the exchanges."""
    from tests import _hostmath as hm
    if not hm.available():
        pytest.skip("hipcc (used as host C++ compiler) missing")
    cls = hm.make_engine_class()
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_newton_worker, args=(r, world, port, q, n))
             for r in range(world)]
    for p in procs:
        p.start()
    results = sorted([q.get(timeout=200) for _ in range(world)], key=lambda t: t[0])
    for p in procs:
        p.join(30)
        assert p.exitcode == 0

    import optiland_amd.tracer as tr
    table = _ref_newton_table()
    eng = cls(table)
    try:
        t = tr.HipRayTracer(table, dtype=torch.float64, engine=eng)
        wl = float(table.wavelengths[0])
        rays = t.trace_generic(*_ref_newton_rays(n), wl)
        want = np.stack([np.asarray(getattr(rays, k))
                         for k in ("x", "y", "z", "L", "M", "N", "opd")])
        if n > 1:   # the point of the exchange: the first shard ALONE stops earlier
            lo, hi = results[0][1], results[0][2]
            alone = t.trace_generic(*[a[lo:hi] for a in _ref_newton_rays(n)], wl)
            assert not np.array_equal(np.asarray(alone.x), want[0, lo:hi])
    finally:
        eng.close()
    got = np.concatenate([r[3] for r in results if r[3] is not None], axis=1)
    assert got.shape == want.shape
    assert np.array_equal(got, want, equal_nan=True)
    assert results[0][4] == results[1][4]
