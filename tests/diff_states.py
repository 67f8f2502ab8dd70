"""States of the step-derivative sweeps (tests/test_diff_sweep_*.py): seeded states of every derivative-supported model
that span every number of penetrating contact points the model can reach, the count per state, and central differences
of the C oracle in one batched call."""
import numpy as np

import tds_amd
import oraclelib  # checker only
import reflib  # checker only
from test_oct import _contact_states

# the largest number of contact points each model can have penetrating at once (plane contacts only)
MAX_CONTACTS = {"ant": 17, "ant_floating": 9, "laikago": 4, "laikago_soft": 4, "laikago_floating": 4,
                "laikago_floating_env": 4, "cube_floating": 8, "pendulum5_plane": 5, "cartpole_plane": 6}
MODELS = list(MAX_CONTACTS)
LAIKAGO = ("laikago", "laikago_soft", "laikago_floating", "laikago_floating_env")


def _unit_quats(rng, n, spread):
    """[n, 4] unit quaternions (x, y, z, w) around the identity"""
    q = rng.normal(size=(n, 4)) * [spread, spread, spread, 0.0] + [0.0, 0.0, 0.0, 1.0]
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def _ant(m, n, rng):
    """test_oct's spread from lying inside the plane to airborne, a quarter of it flat and sunk (all 17 points down)"""
    k = n // 4
    x = _contact_states(m, n, rng, lo=0.0, hi=0.75, tilt=1.2)
    x[:k, 2] = rng.uniform(-0.1, 0.02, k)
    x[:k, 3:5] *= 0.05
    return x


def _ant_floating(m, n, rng):
    """the golden recipe of the floating Ant (TAU mode: q = [quat | pos | joints]) from sunk to airborne"""
    nq, nd = m.dof_q, m.dof_qd
    x = np.zeros((n, m.input_dim))
    x[:, 0:4] = _unit_quats(rng, n, 0.3)
    x[:, 4:6] = rng.uniform(-1, 1, (n, 2))
    x[:, 6] = rng.uniform(-0.1, 0.6, n)
    x[:, 7:nq] = rng.uniform(-0.6, 0.6, (n, nq - 7))
    x[:, nq:nq + nd] = rng.uniform(-1, 1, (n, nd))
    x[:, nq + nd:] = rng.uniform(-1, 1, (n, m.action_dim))
    k = n // 4
    x[:k, 0:4] = _unit_quats(rng, k, 0.02)
    x[:k, 6] = rng.uniform(-0.1, 0.0, k)
    x[:k, 7:nq] *= 0.1
    return x


def _laikago(m, n, rng):
    """test_quad's contact-pattern recipe (0 .. 4 toes down); the floating bases carry the tilt as a quaternion"""
    nq, nd, adim = m.dof_q, m.dof_qd, m.action_dim
    x = np.zeros((n, m.input_dim))
    ip = np.array([m.initial_poses[i] for i in range(adim)])
    if m.is_floating:
        x[:, 0:4] = _unit_quats(rng, n, 0.2)
        x[:, 4:6] = rng.uniform(-2, 2, (n, 2))
        x[:, 6] = rng.uniform(0.30, 0.50, n)
        j0 = 7
    else:
        x[:, 0:2] = rng.uniform(-2, 2, (n, 2))
        x[:, 2] = rng.uniform(0.30, 0.50, n)        # from well inside the plane to airborne
        x[:, 3:5] = rng.uniform(-0.4, 0.4, (n, 2))  # roll / pitch: some toes down, some up
        x[:, 5] = rng.uniform(-3, 3, n)
        j0 = 6
    x[:, j0:nq] = (ip if m.step_mode == tds_amd.TDS_STEP_LOCOMOTION else 0.0) + rng.uniform(-0.5, 0.5, (n, nq - j0))
    x[:, nq:nq + nd] = rng.uniform(-1.5, 1.5, (n, nd))
    if m.step_mode == tds_amd.TDS_STEP_LOCOMOTION:
        x[:, nq + nd:nq + nd + adim] = rng.uniform(-0.4, 0.4, (n, adim))
        x[:, -3:] = [100, 2, 50]
    else:
        x[:, nq + nd:] = rng.uniform(-1, 1, (n, m.input_dim - nq - nd))
    return x


def _cube(m, n, rng):
    """a free cube (8 corner spheres) from sunk and level (every corner down) over tilted (1 .. 7) to airborne"""
    nq, nd = m.dof_q, m.dof_qd
    x = np.zeros((n, m.input_dim))
    x[:, 0:4] = _unit_quats(rng, n, 0.35)
    x[:, 4:6] = rng.uniform(-1, 1, (n, 2))
    x[:, 6] = rng.uniform(-0.45, 0.7, n)
    x[:, nq:nq + nd] = rng.uniform(-1, 1, (n, nd))
    k = n // 8
    x[:k, 0:4] = _unit_quats(rng, k, 0.01)       # level: 0, 4 or 8 corners
    x[:k, 6] = rng.uniform(-0.45, 0.6, k)
    return x


def _pendulum5_plane(m, n, rng):
    """the chain lies along +y in the plane z = 0 at q = 0: small angles straddle the ground (golden recipe)"""
    nq, nd = m.dof_q, m.dof_qd
    x = np.zeros((n, m.input_dim))
    x[:, :nq] = rng.uniform(-0.25, 0.25, (n, nq))
    x[: n // 8, :nq] *= 0.02                     # nearly flat: every sphere down
    x[:, nq:nq + nd] = rng.uniform(-1, 1, (n, nd))
    x[:, nq + nd:] = rng.uniform(-1, 1, (n, nd))
    return x


def _cartpole_plane(m, n, rng):
    nq, nd = m.dof_q, m.dof_qd
    x = np.zeros((n, m.input_dim))
    x[:, :nq] = rng.uniform(-1, 1, (n, nq))
    x[:, nq:nq + nd] = rng.uniform(-1, 1, (n, nd))
    x[:, nq + nd:] = rng.uniform(-1, 1, (n, nd)) * 10
    return x


_RECIPES = {"ant": _ant, "ant_floating": _ant_floating, "cube_floating": _cube, "pendulum5_plane": _pendulum5_plane,
            "cartpole_plane": _cartpole_plane}


def states(name, n, seed=0, m=None):
    """n seeded states [n, input_dim] of model `name` spanning its contact counts"""
    m = m if m is not None else tds_amd.load_model(name)
    rng = np.random.default_rng(seed)
    return (_laikago if name in LAIKAGO else _RECIPES[name])(m, n, rng)


def contact_counts(name, m, x, reference=True):
    """penetrating contact points of each state [n]: the reference's own count (last_penetrating_contacts) where its
    library is built and `reference` is set, otherwise the oracle's narrowphase (distance < 0, as the step decides
    `hit`).  The GPU tests pass reference=False: the reference's sources and data are not there."""
    x = np.atleast_2d(x)
    out = np.zeros(x.shape[0], dtype=np.int64)
    if reference and reflib.available():
        import gen_golden  # checker only: the table of reference constructors

        r, _ = gen_golden.make_ref(name)
        try:
            for e in range(x.shape[0]):
                r.step(x[e:e + 1])
                out[e] = sum(r.last_penetrating_contacts())
        finally:
            r.close()
        return out
    for e in range(x.shape[0]):
        out[e] = int((oraclelib.step_debug(m, x[e])["contacts"][:, 9] < 0).sum())
    return out


def histogram(counts, top):
    return np.bincount(counts, minlength=top + 1)


def oracle_step(m):
    return lambda z: oraclelib.step(m, z, threads=min(16, oraclelib.max_threads()))


def central_jacobian(m, x, cols=None, h_rel=1e-6, kink_tol=1e-5, step=None):
    """central differences of the oracle's step (or of `step`) at every state x [n, input_dim] over the input columns
    `cols` (all by default), h = h_rel max(1, |x_j|), from ONE step call on [x | x +- h e_j | x +- 2h e_j].  Returns
    (J [n, output_dim, len(cols)], kink [n]): kink where a column's forward and backward one-sided differences disagree
    by more than kink_tol relative to max(1, max |J|) of the state, i.e. a branch switches within +- 2h.  The one-sided
    differences are the second-order ones, (-3 y0 + 4 y(+h) - y(+2h)) / 2h and its mirror: on a smooth stretch they
    agree to O(h^2), where the first-order pair would differ by h f'' and flag the stiff contact states as kinks."""
    x = np.atleast_2d(np.asarray(x, dtype=np.float64))
    n, nin = x.shape
    cols = np.arange(nin) if cols is None else np.asarray(cols)
    c = cols.size
    h = h_rel * np.maximum(1.0, np.abs(x[:, cols]))            # [n, c]
    batch = np.repeat(x[:, None, :], 1 + 4 * c, axis=1)        # [n, 1 + 4c, nin]
    idx = np.arange(c)
    for s, mult in enumerate((1.0, -1.0, 2.0, -2.0)):
        batch[:, 1 + s * c + idx, cols] += mult * h
    f = step if step is not None else oracle_step(m)
    y = f(batch.reshape(-1, nin)).reshape(n, 1 + 4 * c, -1)
    y0, yp, ym, yp2, ym2 = y[:, :1], y[:, 1:1 + c], y[:, 1 + c:1 + 2 * c], y[:, 1 + 2 * c:1 + 3 * c], y[:, 1 + 3 * c:]
    return _central_and_kink(y0, yp, ym, yp2, ym2, h[:, :, None], kink_tol)


def _central_and_kink(y0, yp, ym, yp2, ym2, hh, kink_tol):
    """y* [n, c, output_dim] at 0, +h, -h, +2h, -2h; hh broadcasts against them"""
    J = ((yp - ym) / (2 * hh)).transpose(0, 2, 1)
    fwd = (-3 * y0 + 4 * yp - yp2) / (2 * hh)
    bwd = (3 * y0 - 4 * ym + ym2) / (2 * hh)
    scale = np.maximum(1.0, np.abs(J).max(axis=(1, 2)))
    kink = np.abs(fwd - bwd).max(axis=2) / scale[:, None] > kink_tol   # [n, c]
    return J, kink.any(axis=1)


def central_theta(m, x, sel, step_of_model, set_param, h_rel=1e-6, kink_tol=1e-5):
    """central differences over the selected model scalars `sel` (param_spec tuples), each on model copies made by
    set_param(m, q, value); step_of_model(model, x) -> y; h = h_rel |theta_j| (h_rel where theta_j = 0: a light link's
    mass takes a step of its own size).  Returns (J [n, output_dim, p], kink [n, p])."""
    from tds_amd import hip_backend as hb

    theta = hb.params_get(m, sel)
    y0 = step_of_model(m, x)[:, None]
    J, kink = [], []
    for j, q in enumerate(sel):
        h = h_rel * (abs(theta[j]) or 1.0)
        ys = [step_of_model(set_param(m, q, theta[j] + s * h), x)[:, None] for s in (1, -1, 2, -2)]
        Jj, kj = _central_and_kink(y0, *ys, h, kink_tol)
        J.append(Jj)
        kink.append(kj)
    return np.concatenate(J, axis=2), np.stack(kink, axis=1)
