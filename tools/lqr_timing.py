"""Times, in one process, the two native pieces of batched iLQR next to what a user composes from public calls without
them, and the split of one iLQR iteration.

  lqr_backward       against the same recursion from torch.bmm / torch.linalg.cholesky_ex / torch.cholesky_solve, same
                     inputs: problem sets of the Ant's size (nx 28, nu 8) and of the largest (nx 40, nu 16), T 64,
                     n 64 / 1024 / 4096
  feedback_rollout   against T rounds of forward_zero with the feedback law in torch ops (Ant, T 64, rows 64 / 1024 / 4096)
  one ilqr iteration Ant, 64 problems, T 64, 8 alphas: linearisation (jacobian), backward pass, line-search rollout
  lqr_backward_box   (--sections box) against lqr_backward on the same problem sets, once with infinite bounds and once
                     with bounds at half the unconstrained k on a random half of the controls: `ratio` = slowest box /
                     fastest plain, the mean QP iterations and the share of clamped controls; then one
                     ilqr(u_limits="model") iteration on the Ant beside the unlimited one

Per case a warm-up call, then `--reps` calls timed one by one (a synchronise around each): the line gives the slowest
and fastest of each side and `ratio` = slowest native / fastest yardstick (the requirement is ratio <= 1).  Run it
under `rocprofv3 --kernel-trace --stats -- python tools/lqr_timing.py` for the kernels' own durations
(profiles/lqr_timing.txt quotes both)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--T", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="64,1024,4096")
    ap.add_argument("--sections", default="plain", help="comma-separated: plain (the yardstick comparisons), box")
    args = ap.parse_args()

    import numpy as np
    import torch

    import tds_amd
    from tds_amd import hip_backend as hb

    T, dev = args.T, "cuda"
    sizes = [int(s) for s in args.sizes.split(",") if s]
    m = tds_amd.load_model("ant")
    nsd, n_act, _ = hb.trajectory_dims(m, 1)
    sim = hb.HipSim(m, max(sizes), device=0, dtype="f64")
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64, device=dev)  # noqa: E731

    def times(fn):
        fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    def report(case, native, yard, **extra):
        print(json.dumps(dict({"case": case, "native_ms": [round(min(native), 3), round(max(native), 3)],
                               "yardstick_ms": [round(min(yard), 3), round(max(yard), 3)],
                               "ratio": round(max(native) / min(yard), 4)}, **extra)), flush=True)

    def spd(n, t, d):
        a = rnd(n, t, d, d) / d ** 0.5
        return a @ a.transpose(-1, -2) + torch.eye(d, dtype=torch.float64, device=dev)

    def composed_backward(A, B, lx, lu, lxx, luu, lux, mu):
        n, T_, nx, nu = B.shape
        Vx, Vxx = lx[:, T_, :, None], lxx[:, T_]
        eye = torch.eye(nu, dtype=torch.float64, device=dev) * mu[:, None, None]
        k, K = torch.empty((n, T_, nu), dtype=torch.float64, device=dev), torch.empty((n, T_, nu, nx), dtype=torch.float64, device=dev)
        dv1 = torch.zeros(n, dtype=torch.float64, device=dev)
        dv2 = torch.zeros(n, dtype=torch.float64, device=dev)
        bad = torch.zeros(n, dtype=torch.int32, device=dev)
        for t in range(T_ - 1, -1, -1):
            a, b = A[:, t], B[:, t]
            at, bt = a.transpose(1, 2), b.transpose(1, 2)
            Qx, Qu = lx[:, t, :, None] + torch.bmm(at, Vx), lu[:, t, :, None] + torch.bmm(bt, Vx)
            VA = torch.bmm(Vxx, a)
            Qxx, Qux, Quu = lxx[:, t] + torch.bmm(at, VA), lux[:, t] + torch.bmm(bt, VA), luu[:, t] + torch.bmm(bt, torch.bmm(Vxx, b))
            L, info = torch.linalg.cholesky_ex(Quu + eye)
            bad = torch.where((bad == 0) & (info != 0), t + 1, bad)
            sol = -torch.cholesky_solve(torch.cat([Qu, Qux], dim=2), L)
            kk, KK = sol[:, :, :1], sol[:, :, 1:]
            KKt = KK.transpose(1, 2)
            Vx = Qx + torch.bmm(KKt, torch.bmm(Quu, kk)) + torch.bmm(KKt, Qu) + torch.bmm(Qux.transpose(1, 2), kk)
            Vxx = Qxx + torch.bmm(KKt, torch.bmm(Quu, KK)) + torch.bmm(KKt, Qux) + torch.bmm(Qux.transpose(1, 2), KK)
            Vxx = 0.5 * (Vxx + Vxx.transpose(1, 2))
            dv1 += (kk * Qu).sum(dim=(1, 2))
            dv2 += 0.5 * (kk * torch.bmm(Quu, kk)).sum(dim=(1, 2))
            k[:, t], K[:, t] = kk[:, :, 0], KK
        return k, K, torch.stack([dv1, dv2], dim=1), bad

    sections = [w for w in args.sections.split(",") if w]

    def problems(n, nx, nu):
        A = rnd(n, T, nx, nx) / nx ** 0.5
        B = rnd(n, T, nx, nu) / nx ** 0.5
        return (A, B, rnd(n, T + 1, nx), rnd(n, T, nu), spd(n, T + 1, nx), spd(n, T, nu), 0.1 * rnd(n, T, nu, nx),
                torch.full((n,), 1e-6, dtype=torch.float64, device=dev))

    if "box" in sections:
        box_section(args, sim, m, sizes, problems, times, rnd)
    if "plain" not in sections:
        return

    for nx, nu in ((nsd, n_act), (hb.LQR_MAX_NX, hb.LQR_MAX_NU)):
        for n in sizes:
            P = problems(n, nx, nu)
            A, B = P[:2]
            got, want = sim.lqr_backward(*P), composed_backward(*P)
            diff = max(float((g - w).abs().max() / w.abs().max().clamp(min=1.0)) for g, w in zip(got[:3], want[:3]))
            report(f"lqr_backward nx={nx} nu={nu} T={T} n={n}", times(lambda: sim.lqr_backward(*P)),
                   times(lambda: composed_backward(*P)), max_rel_diff=diff, status_equal=bool(torch.equal(got[3], want[3])))
            del P, A, B, got, want

    g = np.load(os.path.join(ROOT, "tests", "golden", "ant.npz"))["x"]
    rng = np.random.default_rng(0)

    def composed_rollout(sim, x0, s_nom, u_nom, k, K, alpha):
        x = x0.clone()
        ss, uu = [x0[:, :nsd]], []
        for t in range(T):
            s = x[:, :nsd]
            u = (u_nom[:, t] + alpha[:, None] * k[:, t]) + torch.bmm(K[:, t], (s - s_nom[:, t])[:, :, None])[:, :, 0]
            x = torch.cat([s, u, x0[:, nsd + n_act:]], dim=1)
            x = torch.cat([sim.forward_zero(x)[:, :nsd], x[:, nsd:]], dim=1)
            ss.append(x[:, :nsd])
            uu.append(u)
        return torch.stack(ss, dim=1), torch.stack(uu, dim=1)

    for n in sizes:
        roll = hb.HipSim(m, n, device=0, dtype="f64")  # (forward_zero serves exactly num_envs records)
        x0 = torch.from_numpy(g[rng.integers(0, g.shape[0], n)]).to(dev)
        s_nom = x0[:, None, :nsd] + 0.01 * rnd(n, T + 1, nsd)
        u_nom, k, K = 0.1 * rnd(n, T, n_act), 0.01 * rnd(n, T, n_act), 0.01 * rnd(n, T, n_act, nsd)
        alpha = torch.ones(n, dtype=torch.float64, device=dev)
        Pr = (x0, s_nom, u_nom, k, K, alpha)
        report(f"feedback_rollout ant T={T} rows={n}", times(lambda: roll.feedback_rollout(*Pr)),
               times(lambda: composed_rollout(roll, *Pr)))
        roll.close()

    # one iLQR iteration, Ant x 64, T 64, the default 8 alphas
    N, C = 64, 8
    sim64 = hb.HipSim(m, N * C, device=0, dtype="f64")
    x0 = torch.from_numpy(g[rng.integers(0, g.shape[0], N)]).to(dev)
    u0 = 0.1 * rnd(N, T, n_act)
    z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)  # noqa: E731
    s, u = sim64.feedback_rollout(x0, z(N, T + 1, nsd), u0, z(N, T, n_act), z(N, T, n_act, nsd), z(N))
    cost = tds_amd.QuadraticCost(torch.eye(nsd), 0.1 * torch.eye(n_act), torch.eye(nsd))
    rec = hb.trajectory_records(m, x0, s, u)
    lin = times(lambda: sim64.jacobian(rec, rows=range(nsd), cols=range(nsd + n_act)))
    jac = sim64.jacobian(rec, rows=range(nsd), cols=range(nsd + n_act)).reshape(N, T, nsd, nsd + n_act)
    A, B = jac[..., :nsd].contiguous(), jac[..., nsd:].contiguous()
    _, lx, lu, lxx, luu, lux = cost.expand(s, u)
    mu = torch.full((N,), 1e-6, dtype=torch.float64, device=dev)
    back = times(lambda: sim64.lqr_backward(A, B, lx, lu, lxx, luu, lux, mu))
    k, K, dv, status = sim64.lqr_backward(A, B, lx, lu, lxx, luu, lux, mu)
    por = torch.arange(N, dtype=torch.int32, device=dev).repeat_interleave(C)
    al = torch.tensor([2.0 ** -i for i in range(C)], dtype=torch.float64, device=dev).repeat(N)
    x0r = x0.repeat_interleave(C, dim=0)
    line = times(lambda: sim64.feedback_rollout(x0r, s, u, k, K, al, por, check=False))
    whole = times(lambda: tds_amd.ilqr(sim64, x0, u0, cost, iterations=1))
    rng_ms = lambda t: [round(min(t), 3), round(max(t), 3)]  # noqa: E731
    print(json.dumps({"case": f"one ilqr iteration, ant x {N}, T={T}, {C} alphas", "linearisation_ms": rng_ms(lin),
                      "backward_pass_ms": rng_ms(back), "line_search_rollout_ms": rng_ms(line),
                      "ilqr_iterations_1_ms (with the first open-loop rollout)": rng_ms(whole),
                      "status_nonzero": int((status != 0).sum())}), flush=True)


def box_section(args, sim, m, sizes, problems, times, rnd):
    import numpy as np
    import torch

    import tds_amd
    from tds_amd import hip_backend as hb

    T, dev = args.T, "cuda"
    nsd, n_act, _ = hb.trajectory_dims(m, 1)
    rng_ms = lambda t: [round(min(t), 3), round(max(t), 3)]  # noqa: E731
    for nx, nu in ((nsd, n_act), (hb.LQR_MAX_NX, hb.LQR_MAX_NU)):
        for n in sizes:
            P = problems(n, nx, nu)
            k = sim.lqr_backward(*P)[0]
            inf = torch.full((n, T, nu), float("inf"), dtype=torch.float64, device=dev)
            # half the controls, chosen at random, may move half as far as the unconstrained pass would move them
            cut = torch.rand((n, T, nu), device=dev, generator=torch.Generator(device=dev).manual_seed(n + nu)) < 0.5
            dlo = torch.where(cut & (k < 0), 0.5 * k, -inf)
            dhi = torch.where(cut & (k > 0), 0.5 * k, inf)
            plain = times(lambda: sim.lqr_backward(*P))
            for what, lo, hi in (("infinite bounds", -inf, inf), ("half cut", dlo, dhi)):
                box = times(lambda: sim.lqr_backward_box(*P, lo, hi, check=False))
                res = sim.lqr_backward_box(*P, lo, hi, check=False)
                share = float(sum(((res[4] >> a) & 1).double().mean() for a in range(nu)) / nu)
                print(json.dumps({"case": f"lqr_backward_box nx={nx} nu={nu} T={T} n={n}, {what}",
                                  "box_ms": rng_ms(box), "plain_ms": rng_ms(plain),
                                  "ratio": round(max(box) / min(plain), 4),
                                  "mean_qp_iterations": round(float(res[5].double().mean()), 3),
                                  "clamped_share": round(share, 3), "status_nonzero": int((res[3] != 0).sum())}),
                      flush=True)
            del P, k, inf, cut, dlo, dhi
    # one iLQR iteration on the Ant with and without the model's limits
    N, C = 64, 8
    g = np.load(os.path.join(ROOT, "tests", "golden", "ant.npz"))["x"]
    sim64 = hb.HipSim(m, N * C, device=0, dtype="f64")
    x0 = torch.from_numpy(g[np.random.default_rng(0).integers(0, g.shape[0], N)]).to(dev)
    u0 = 0.3 * rnd(N, T, n_act)
    cost = tds_amd.QuadraticCost(torch.eye(nsd), 0.1 * torch.eye(n_act), torch.eye(nsd))
    free = times(lambda: tds_amd.ilqr(sim64, x0, u0, cost, iterations=1))
    lim = times(lambda: tds_amd.ilqr(sim64, x0, u0, cost, iterations=1, u_limits="model"))
    r = tds_amd.ilqr(sim64, x0, u0, cost, iterations=1, u_limits="model")
    print(json.dumps({"case": f"one ilqr iteration, ant x {N}, T={T}, {C} alphas (with the first open-loop rollout)",
                      "unlimited_ms": rng_ms(free), "model_limits_ms": rng_ms(lim),
                      "ratio": round(max(lim) / min(free), 4),
                      "mean_qp_iterations": round(float(r["qp_iterations"].double().mean()), 3),
                      "steps_with_a_clamped_control": int((r["clamped"] != 0).sum()), "steps": N * T,
                      "accepted": int((r["alpha"] > 0).sum())}), flush=True)
    sim64.close()


if __name__ == "__main__":
    main()
