"""CPU: the step derivatives' template (tds_diff_step.h) over seeded sweeps that span every contact count each model can
reach (tests/diff_states.py), at the models' settings and on copies with pgs_iterations 2 and 3 and with friction 0:
the primal against the C oracle (and the reference where it is built), the forward-mode tangents and theta columns
against central differences of the oracle, forward against reverse mode, the reverse-mode tapes against their class
capacity, and the pgs_iterations boundary of the Ant's reverse mode."""
import ctypes as C
import functools

import numpy as np
import pytest

import tds_amd
from tds_amd import hip_backend as hb
import diff_states as ds
import oraclelib  # checker only
import reflib  # checker only
from test_param_derivs_cpu import set_param

SETTINGS = {"default": {}, "pgs2": {"pgs_iterations": 2}, "pgs3": {"pgs_iterations": 3}, "friction0": {"friction": 0.0}}
SWEEP = {"ant": 400}  # states per model; others: 300
ANT_PGS_FIT = (1, 2, 3)  # pgs_iterations whose Ant tapes fit class A's capacity on the sweep
ANT_PGS_OVERFLOW = 4     # the first that does not
# the largest pgs_iterations whose tapes fit on the sweep of the model that binds its class (plain, every parameter
# selected); each further PGS sweep lengthens a tape by a fixed count
PGS_RANGE = {"pendulum5_plane": (7, 8), "ant": (3, 3), "laikago": (11, 9)}


def model(name, setting="default"):
    m = tds_amd.load_model(name).copy()
    for k, v in SETTINGS[setting].items():
        setattr(m, k, v)
    return m


@functools.lru_cache(maxsize=None)
def sweep(name):
    """(x, contact counts) of the model's sweep; the counts do not depend on the solver settings"""
    m = tds_amd.load_model(name)
    x = ds.states(name, SWEEP.get(name, 300), seed=1, m=m)
    x.setflags(write=False)
    return x, ds.contact_counts(name, m, x)


def step_rel(y, y_ref):
    """per-step relative error, floor 1 (tests/test_jacobian_cpu.py)"""
    return float(np.max(np.abs(y - y_ref) / np.maximum(np.abs(y_ref), 1.0)))


def state_rel(a, b):
    """per state: max |a - b| / max(1, max |b|)"""
    ax = tuple(range(1, a.ndim))
    return np.abs(a - b).max(axis=ax) / np.maximum(1.0, np.abs(b).max(axis=ax))


def theta_sel(m, setting):
    """friction, restitution, gravity x / z and the heaviest link's mass (friction left out at friction 0: the box
    [-mu pn, mu pn] closes there, a kink)"""
    heavy = max(range(m.num_links), key=lambda i: m.links[i].mass) if m.num_links else None
    sel = [("restitution",), ("gravity", 0), ("gravity", 2), ("mass", heavy) if m.num_links else ("base_mass",)]
    return sel if setting == "friction0" else [("friction",)] + sel


@pytest.mark.parametrize("name", ds.MODELS)
def test_contact_histogram_reaches_the_maximum(name, built):
    _, counts = sweep(name)
    hist = ds.histogram(counts, ds.MAX_CONTACTS[name])
    print(f"{name}: {counts.size} states, penetrating contacts histogram {hist.tolist()}")
    assert counts.max() == ds.MAX_CONTACTS[name] and hist[-1] >= 5, hist
    if name != "cartpole_plane":  # (the cart rides at a fixed height: the same points always)
        assert hist[0] >= 5 and np.count_nonzero(hist) >= 0.8 * hist.size, hist


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name", ds.MODELS)
def test_primal_matches_the_oracle(name, setting, built):
    m = model(name, setting)
    x, _ = sweep(name)
    y_ref = oraclelib.step(m, x)
    y = hb.step_host(m, x)
    _, yj = hb.jacobian_host(m, x[:64], want_y=True)  # the TdsDual instantiation's value part
    _, yv = hb.vjp_host(m, x[:64], np.ones((64, m.output_dim)), want_y=True)  # the TdsRev one's
    assert step_rel(y, y_ref) <= 1e-10
    assert step_rel(yj, y_ref[:64]) <= 1e-10
    assert step_rel(yv, y_ref[:64]) <= 1e-10
    if reflib.available():  # the reference itself, with the same solver settings
        import gen_golden  # checker only: the table of reference constructors

        r, _ = gen_golden.make_ref(name)
        try:
            r.set_solver(m.cfm, m.erp, m.pgs_iterations, m.friction, m.restitution)
            assert step_rel(y, r.step(x)) <= 1e-10
        finally:
            r.close()


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name", ds.MODELS)
def test_tangents_match_central_differences_of_the_oracle(name, setting, built):
    m = model(name, setting)
    x, counts = sweep(name)
    J = hb.jacobian_host(m, x)
    J_fd, kink = ds.central_jacobian(m, x)
    ok = ~kink
    err = state_rel(J[ok], J_fd[ok])
    checked = np.bincount(counts[ok], minlength=counts.max() + 1)
    present = np.bincount(counts, minlength=counts.max() + 1) > 0
    print(f"{name} [{setting}]: kink-free {ok.mean():.3f}, worst tangent error {err.max():.2e}, "
          f"checked per contact count {checked.tolist()}")
    assert ok.mean() >= 0.9
    assert np.all(checked[present] >= 1)
    assert err.max() <= 1e-7
    # theta columns through jvp_params_host, against the oracle on perturbed model copies
    sel = theta_sel(m, setting)
    nin, p = m.input_dim, len(sel)
    xs = x[::3]
    v = np.zeros((xs.shape[0], p, nin + p))
    v[:, np.arange(p), nin + np.arange(p)] = 1.0
    Jt = hb.jvp_params_host(m, xs, hb.params_get(m, sel), sel, v).transpose(0, 2, 1)
    # (h = 1e-4 |theta|: the model scalars are smooth, and the oracle's rounding over 2h stays below the tolerance)
    Jt_fd, kink_t = ds.central_theta(m, xs, sel, lambda mm, xx: oraclelib.step(mm, xx), set_param, h_rel=1e-4)
    for j, q in enumerate(sel):
        okj = ~kink_t[:, j]
        assert okj.mean() >= 0.9, q
        e = state_rel(Jt[okj][:, :, j], Jt_fd[okj][:, :, j])
        assert e.max() <= 1e-7, (q, e.max())
    assert np.count_nonzero(Jt) > 0


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("name", ds.MODELS)
def test_forward_and_reverse_agree(name, setting, built):
    """w^T (J v) = (w^T J) v in x and in [x | theta] with every selectable parameter"""
    m = model(name, setting)
    x, _ = sweep(name)
    x = x[::4]
    n, nin, nout = x.shape[0], m.input_dim, m.output_dim
    rng = np.random.default_rng(5)
    w = rng.normal(size=(n, nout))

    def check(jv, wj, v):
        a, b = np.einsum("no,no->n", w, jv), np.einsum("ni,ni->n", wj, v)
        scale = np.maximum.reduce([np.ones(n), np.einsum("no,no->n", np.abs(w), np.abs(jv)),
                                   np.einsum("ni,ni->n", np.abs(wj), np.abs(v))])
        assert np.max(np.abs(a - b) / scale) <= 1e-12

    v = rng.normal(size=(n, nin))
    check(np.einsum("noi,ni->no", hb.jacobian_host(m, x), v), hb.vjp_host(m, x, w), v)
    sel = hb.all_params(m)
    theta = hb.params_get(m, sel)
    v = rng.normal(size=(n, nin + len(sel)))
    check(hb.jvp_params_host(m, x, theta, sel, v), hb.vjp_params_host(m, x, theta, sel, w), v)


@pytest.mark.parametrize("name", ds.MODELS)
def test_tapes_fit_the_class_capacity(name, built):
    """every swept state records within its class's capacity (no -1), plain and with every parameter selected"""
    m = model(name)
    x, counts = sweep(name)
    w = np.zeros((x.shape[0], m.output_dim))
    _, lens = hb.vjp_host(m, x, w, tape_len=True)
    sel = hb.all_params(m)
    _, lens_p = hb.vjp_params_host(m, x, hb.params_get(m, sel), sel, w, tape_len=True)
    print(f"{name}: longest tape {lens.max()} (at {counts[np.argmax(lens)]} contacts), every parameter selected "
          f"(p = {len(sel)}) {lens_p.max()}")
    assert np.all(lens > 0) and np.all(lens_p > lens)


@pytest.mark.parametrize("pgs", ANT_PGS_FIT)
def test_ant_reverse_mode_is_exact_within_its_pgs_range(pgs, built):
    m = model("ant")
    m.pgs_iterations = pgs
    x, _ = sweep("ant")
    x = x[::2]
    w = np.random.default_rng(pgs).normal(size=(x.shape[0], 2, m.output_dim))
    wj, y, lens = hb.vjp_host(m, x, w, want_y=True, tape_len=True)
    jac, yj = hb.jacobian_host(m, x, want_y=True)
    ref = np.einsum("nko,noi->nki", w, jac)
    assert np.all(lens > 0)
    assert np.max(state_rel(wj, ref)) <= 1e-11
    assert step_rel(y, yj) <= 1e-12
    sel = hb.all_params(m)
    _, lens_p = hb.vjp_params_host(m, x, hb.params_get(m, sel), sel, w, tape_len=True)
    print(f"ant, pgs_iterations {pgs}: longest tape {lens.max()}, every parameter selected {lens_p.max()}")
    assert np.all(lens_p > 0)


def test_ant_reverse_mode_fails_cleanly_past_its_pgs_range(built):
    """at the first pgs_iterations whose tapes overflow class A: the capacity error, NaN y / wj for exactly the
    environments that overflowed and the exact result for the rest (raw C call); forward mode stays exact there"""
    m = model("ant")
    m.pgs_iterations = ANT_PGS_OVERFLOW
    x_all, counts = sweep("ant")
    # (a host cap of 2^18 entries, 8 MB per tape: room for every state, which -1 would show otherwise)
    _, lens_unbounded = hb.vjp_host(m, x_all, np.zeros((x_all.shape[0], m.output_dim)), tape_len=True,
                                    tape_cap=1 << 18)
    assert np.all(lens_unbounded > 0)
    fits, over = int(np.argmin(lens_unbounded)), int(np.argmax(lens_unbounded))
    print(f"ant, pgs_iterations {ANT_PGS_OVERFLOW}: tapes {lens_unbounded.min()} .. {lens_unbounded.max()}")
    x = np.ascontiguousarray(x_all[[fits, over]])
    w = np.random.default_rng(7).normal(size=(2, m.output_dim))
    with pytest.raises(hb.TdsHipError, match="tape exceeds the capacity"):
        hb.vjp_host(m, x, w)
    wj = np.zeros((2, m.input_dim))
    y = np.zeros((2, m.output_dim))
    got = np.zeros(2, dtype=np.int32)
    rc = hb.lib().tds_hip_vjp_host_tape(C.byref(m), 2, x.ctypes.data, 1, w.ctypes.data, y.ctypes.data,
                                        wj.ctypes.data, 0, got.ctypes.data)
    assert rc == 2  # TDS_ERR_UNSUPPORTED
    assert got[0] == lens_unbounded[fits] and got[1] == -1
    assert np.all(np.isnan(wj[1])) and np.all(np.isnan(y[1]))
    jac, yj = hb.jacobian_host(m, x, want_y=True)
    np.testing.assert_allclose(wj[0], w[0] @ jac[0], rtol=0, atol=1e-11 * max(1.0, np.abs(wj[0]).max()))
    # forward mode: the primal and the tangents over the whole sweep
    x_all = x_all[::2]
    jac, yj = hb.jacobian_host(m, x_all, want_y=True)
    assert step_rel(yj, oraclelib.step(m, x_all)) <= 1e-10
    J_fd, kink = ds.central_jacobian(m, x_all)
    assert (~kink).mean() >= 0.9
    assert np.max(state_rel(jac[~kink], J_fd[~kink])) <= 1e-7


@pytest.mark.parametrize("name", list(PGS_RANGE))
def test_pgs_iterations_range_of_each_class(name, built):
    """S (pendulum5_plane), A (ant) and L (laikago) bind their classes' capacities: every swept state fits at the
    documented largest pgs_iterations, and one more overflows, in plain and in parameter mode"""
    x, _ = sweep(name)
    for params, last in zip((False, True), PGS_RANGE[name]):
        for pgs, fits in ((last, True), (last + 1, False)):
            m = model(name)
            m.pgs_iterations = pgs
            w = np.zeros((x.shape[0], m.output_dim))
            if params:
                sel = hb.all_params(m)
                call = lambda: hb.vjp_params_host(m, x, hb.params_get(m, sel), sel, w, tape_len=True)  # noqa: E731
            else:
                call = lambda: hb.vjp_host(m, x, w, tape_len=True)  # noqa: E731
            if fits:
                _, lens = call()
                print(f"{name}, pgs_iterations {pgs}{' (every parameter)' if params else ''}: longest tape {lens.max()}")
                assert np.all(lens > 0)
            else:
                with pytest.raises(hb.TdsHipError, match="tape exceeds the capacity"):
                    call()
