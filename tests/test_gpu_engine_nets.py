"""The replica engine on the networks its lock-step schedule took last: the two wide shapes on the bf16 matrix
cores (BASELINE config 5's 32->128-128-1, config 3's 16->64-64-64-1) and a float32 network too large for one
workgroup's LDS (8->256-256-1: tests/test_stream_host.py pins its mask at 7).  The C++ host loop against the Python
statement bit for bit, both against the CPU oracle within the tolerances tests/test_gpu_parity.py states for the fit
kernels, sharding, and the asynchronous schedule's refusal.  Everything here needs an MI355X."""
import numpy as np
import pytest

from bore_amd import _lib, ops, shuffle
from bore_amd.engine import NativeEngine, ReplicaEngine, ShardedEngine
from oracle import bore_oracle as O

pytestmark = pytest.mark.gpu

NETS = {
    "bf16-32x128": dict(input_dim=32, units=(128, 128, 1), acts=("relu", "relu", "linear"), compute="bfloat16"),
    "bf16-16x64": dict(input_dim=16, units=(64, 64, 64, 1), acts=("relu", "relu", "relu", "linear"),
                       compute="bfloat16"),
    "streamed-8x256": dict(input_dim=8, units=(256, 256, 1), acts=("relu", "relu", "linear"), compute="float32"),
}
IDS = np.arange(3, 8)           # five loops: groups=2 splits them 2 / 3
GAMMA, N_INIT, SEED = 0.25, 10, 0


def quadratic(X):
    return np.sum((X - 0.3) ** 2, axis=-1)


COMMON = dict(n_init=N_INIT, epochs=3, num_samples=64, num_starts=3, options=dict(maxiter=30, ftol=1e-9),
              deduplicate=True, objective=quadratic, gamma=GAMMA, seed=SEED)


def unpack(flat, D, units):
    out, off, k = [], 0, D
    for u in units:
        out.append(flat[off:off + k * u].reshape(k, u).copy()); off += k * u
        out.append(flat[off:off + u].copy()); off += u
        k = u
    return out


def pack(params):
    return np.concatenate([np.asarray(p, dtype=np.float32).reshape(-1) for p in params])


_native = {}


def native_run(name):
    """NativeEngine(groups=2) after run(2) + run(2), once per network: (X, y, state, stats)."""
    if name not in _native:
        a = NativeEngine(IDS, groups=2, **NETS[name], **COMMON)
        th0 = a.state()[0]
        a.run(2)
        a.run(2)
        X, y = a.observations()
        _native[name] = dict(X=X, y=y, th0=th0, state=a.state(), stats=a.take_stats())
        a.close()
    return _native[name]


@pytest.mark.parametrize("name", list(NETS))
def test_native_engine_equals_python_engine(gpu, name):
    """The form of tests/test_gpu_argmax.py's test of the same name, on the new networks."""
    a = native_run(name)
    b = ReplicaEngine(IDS, mode="device", groups=1, **NETS[name], **COMMON)
    assert b.N == N_INIT and np.array_equal(a["X"][:, :N_INIT], b.X)
    b.run(2)
    b.run(2)
    D = NETS[name]["input_dim"]
    assert a["X"].shape == (5, N_INIT + 4, D)
    assert np.array_equal(a["X"], b.X) and np.array_equal(a["y"], b.y)
    th, m, v, t = a["state"]
    assert np.array_equal(th, b.theta.cpu().numpy()) and np.array_equal(t, b.adam_t.cpu().numpy())
    assert np.array_equal(v, b.adam_v.cpu().numpy())
    assert np.all(t == 4 * 3)                                        # (one batch per epoch at these sizes)
    st = a["stats"]
    assert st["none_results"] == b.stats["none_results"] and st["n_fg_rows"] == b.stats["n_fg_rows"]
    assert st["fit_launches"] == 2 * 4 and st["fit_ms"] > 0 and st["argmax_ms"] > 0
    assert not np.array_equal(th, a["th0"])


@pytest.mark.parametrize("name", list(NETS))
def test_host_selection_gives_the_same_observations(gpu, name):
    a = native_run(name)
    b = ReplicaEngine(IDS, mode="device", groups=1, select="host", **NETS[name], **COMMON)
    b.run(2)
    b.run(2)
    assert np.array_equal(a["X"], b.X) and np.array_equal(a["y"], b.y)


@pytest.mark.parametrize("name", ["bf16-32x128", "bf16-16x64"])
def test_bf16_engine_is_not_float32_in_disguise(gpu, name):
    a = native_run(name)
    f = NativeEngine(IDS, groups=2, **dict(NETS[name], compute="float32"), **COMMON)
    assert np.array_equal(f.state()[0], a["th0"])                    # the same start
    f.run(2)
    f.run(2)
    th32 = f.state()[0]
    f.close()
    assert not np.array_equal(th32, a["state"][0])
    assert np.all(np.isfinite(a["state"][0]))


@pytest.mark.parametrize("name", list(NETS))
def test_the_forcing_switch_changes_nothing(gpu, monkeypatch, name):
    """BORE_STREAM=1 sends float32 requests within the bounds to the streamed flavour: the streamed network is
    there already, a bfloat16 one never goes."""
    a = native_run(name)
    if name == "streamed-8x256":
        assert ops.mlp_streamed(_lib.make_desc(8, [256, 256, 1], ["relu", "relu", "linear"])) == 7
        assert a["stats"]["argmax_ms"] > 0
    monkeypatch.setenv("BORE_STREAM", "1")
    b = NativeEngine(IDS, groups=2, **NETS[name], **COMMON)
    b.run(2)
    b.run(2)
    Xb, yb = b.observations()
    stb = b.state()
    b.close()
    assert np.array_equal(a["X"], Xb) and np.array_equal(a["y"], yb)
    for u, v in zip(a["state"], stb):
        assert np.array_equal(u, v)


@pytest.mark.parametrize("name", list(NETS))
def test_first_iteration_tracks_the_oracle(gpu, name):
    """One BO iteration with a 12-epoch fit (12 Adam steps: 10 rows are one batch) against the CPU oracle of every
    loop, from the loop's initial theta, its 10 observations, the labels y < quantile(y, gamma) and the project's
    shuffle stream.  Tolerances as tests/test_gpu_parity.py states them: the bf16 fit over 12 - 24 steps
    atol 1.5e-3 + rtol 2e-2 against oracle.fit_bf16; the float32 fit 5e-6 + 1e-4 |ref| against the float64
    trajectory."""
    net = NETS[name]
    D, units, acts = net["input_dim"], list(net["units"]), list(net["acts"])
    e = NativeEngine(IDS, groups=2, **net, **dict(COMMON, epochs=12))
    th0 = e.state()[0]
    X0, y0 = e.observations()
    assert X0.shape == (5, N_INIT, D)
    e.run(1)
    th, _, _, t = e.state()
    X1, _ = e.observations()
    e.close()
    assert np.all(t == 12)
    x_new = X1[:, N_INIT]
    assert np.all(x_new >= 0.0) and np.all(x_new <= 1.0)             # the first suggestion lies inside the box
    worst = 0.0
    for l, lid in enumerate(IDS):
        z = y0[l] < np.quantile(y0[l], GAMMA)
        perms = shuffle.permutations(SEED, 1, 12, N_INIT, model_index0=int(lid))[0]
        if net["compute"] == "bfloat16":
            ref = unpack(th0[l], D, units)
            st = O.AdamState(ref)
            O.fit_bf16(ref, acts, st, X0[l], z, perms)
            tol = dict(atol=1.5e-3, rtol=2e-2)
        else:
            ref = [p.astype(np.float64) for p in unpack(th0[l], D, units)]
            st = O.AdamState(ref)
            O.fit(ref, acts, st, X0[l].astype(np.float32), z, perms, batch_size=64, dtype=np.float64)
            tol = dict(atol=5e-6, rtol=1e-4)
        assert st.t == 12
        want = pack(ref)
        worst = max(worst, float(np.max(np.abs(th[l] - want) / (tol["atol"] + tol["rtol"] * np.abs(want)))))
        print(f"{name} loop {lid}: |theta - oracle| / tolerance = {worst:.3f}")
        np.testing.assert_allclose(th[l], want, err_msg=f"loop {lid}", **tol)


def test_sharded_engine_equals_one_engine(gpu):
    name = "bf16-32x128"
    a = native_run(name)
    s = ShardedEngine(IDS, shards=2, groups=2, **NETS[name], **COMMON)
    assert len(s.engines) == 2
    s.run(2)
    s.run(2)
    Xs, ys = s.observations()
    ths = s.state()[0]
    s.close()
    assert np.array_equal(a["X"], Xs) and np.array_equal(a["y"], ys)
    assert np.array_equal(a["state"][0], ths)


@pytest.mark.parametrize("name", ["bf16-32x128", "streamed-8x256"])
def test_the_asynchronous_schedule_refuses(gpu, name):
    with pytest.raises(_lib.UnsupportedError, match=r"asynchronous schedule .* \(async_loops = 0\)"):
        NativeEngine(IDS, async_loops=True, **NETS[name], **COMMON)
