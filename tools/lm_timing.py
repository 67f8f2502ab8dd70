"""Times, in one process, the native Levenberg-Marquardt step of batched system identification next to what a user
composes from torch ops without it, and the split of one sysid iteration.

  lm_step            against the same step from torch ops on the same inputs with infinite bounds: the weighted
                     residuals and derivatives, torch.bmm for H and g, then torch.linalg.cholesky_ex +
                     torch.cholesky_solve per candidate (and the same with torch.einsum over rows and entries
                     in place of the transposed copy and the bmm: the ratio is against the faster).  Sizes: 64 problems x 8 rows, m = 100 * 28, p = 9 and 14,
                     L = 5; 4096 problems x 1 row, m = 60 * 10, p = 9, L = 5
  one sysid iteration Ant, 64 problems x 8 rows, T = 100, p = 9, L = 5: the Jacobian call (trajectory_jvp with the p
                     unit directions), the LM step, the candidates' rollout (k = 0, N L copies of the rows) and their
                     costs (the cost-only lm_step)

Per case a warm-up call, then `--reps` calls timed one by one (a synchronise around each): the line gives the slowest
and fastest of each side and `ratio` = slowest native / fastest yardstick (the requirement is ratio <= 1; where it is
missed the line says so and no claim is made).  The lines are printed and written to --out."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lm_timing.txt"))
    args = ap.parse_args()

    import numpy as np
    import torch

    import tds_amd
    from tds_amd import hip_backend as hb

    dev = "cuda"
    m = tds_amd.load_model("ant")
    nsd, n_act, _ = hb.trajectory_dims(m, 1)
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64, device=dev)  # noqa: E731
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

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

    rng_ms = lambda t: [round(min(t), 3), round(max(t), 3)]  # noqa: E731

    def composed(R, s, s_obs, w, js, lam, einsum=False):
        rows, p, mm = js.shape
        n, L = rows // R, lam.shape[1]
        a = (w * (s - s_obs)).reshape(n, R * mm)
        if einsum:  # (no transposed copy of w js: the contraction runs over rows and entries as they lie)
            c = (w[:, None, :] * js).reshape(n, R, p, mm)
            H = torch.einsum("nrpm,nrqm->npq", c, c)
            g = torch.einsum("nrpm,nrm->np", c, a.reshape(n, R, mm))[:, :, None]
        else:
            c = (w[:, None, :] * js).reshape(n, R, p, mm).transpose(1, 2).reshape(n, p, R * mm)
            H, g = torch.bmm(c, c.transpose(1, 2)), torch.bmm(c, a[:, :, None])
        cost = 0.5 * (a * a).sum(dim=1)
        D = torch.diag_embed(H.diagonal(dim1=1, dim2=2).clamp(1e-6, 1e32))
        delta, pred = [], []
        for l in range(L):
            Lc, _ = torch.linalg.cholesky_ex(H + lam[:, l, None, None] * D)
            d = -torch.cholesky_solve(g, Lc)
            delta.append(d[:, :, 0])
            pred.append(-((g * d).sum(dim=(1, 2)) + 0.5 * (d * torch.bmm(H, d)).sum(dim=(1, 2))))
        return cost, g[:, :, 0], H, torch.stack(delta, dim=1), torch.stack(pred, dim=1)

    sim = hb.HipSim(m, 64, device=0, dtype="f64")
    for n, R, mm, p, L in ((64, 8, 100 * 28, 9, 5), (64, 8, 100 * 28, 14, 5), (4096, 1, 60 * 10, 9, 5)):
        rows = n * R
        s, s_obs, js = rnd(rows, mm), rnd(rows, mm), rnd(rows, p, mm)
        w = 0.5 + torch.rand((rows, mm), generator=gen, dtype=torch.float64, device=dev)
        lam = torch.tensor([1e-4 * 3.0 ** (i - 2) for i in range(L)], dtype=torch.float64, device=dev).expand(n, L).contiguous()
        row_start = (torch.arange(n + 1, device=dev) * R).to(torch.int32)
        native = lambda: sim.lm_step(row_start, s, s_obs, js, lam, w, check=False)  # noqa: E731
        got, want = native(), composed(R, s, s_obs, w, js, lam)
        diff = max(float((got[k] - b).abs().max() / b.abs().max().clamp(min=1.0))
                   for k, b in zip(("cost", "g", "H", "delta", "pred"), want))
        tn, ty = times(native), times(lambda: composed(R, s, s_obs, w, js, lam))
        te = times(lambda: composed(R, s, s_obs, w, js, lam, einsum=True))
        ratio = max(tn) / min(ty + te)  # (against the faster of the two compositions)
        emit({"case": f"lm_step n={n} rows/problem={R} m={mm} p={p} L={L}", "native_ms": rng_ms(tn),
              "yardstick_bmm_ms": rng_ms(ty), "yardstick_einsum_ms": rng_ms(te), "ratio": round(ratio, 4),
              "requirement_met": bool(ratio <= 1.0), "max_rel_diff": diff,
              "status_1": int((got["status"] == 1).sum()), "status_2": int((got["status"] == 2).sum()),
              "js_GB_per_s_native": round(js.numel() * 8 / (min(tn) * 1e-3) / 1e9, 1)})
        del s, s_obs, js, w, got, want
    sim.close()

    # one sysid iteration: Ant, 64 problems x 8 rows, T = 100
    N, R, T, L = 64, 8, 100, 5
    sel = [("friction",), ("gravity", 2)] + [("mass", i) for i in range(7)]
    p = len(sel)
    g = np.load(os.path.join(ROOT, "tests", "golden", "ant.npz"))["x"]
    rng = np.random.default_rng(0)
    base = torch.from_numpy(hb.params_get(m, sel)).to(dev)
    sim = hb.HipSim(m, N * L * R, device=0, dtype="f64")
    true = base * torch.from_numpy(rng.uniform(0.9, 1.1, (N, p))).to(dev)
    # Under its record's constant action about one golden record in ten leaves the ground for good within 100 steps
    # (|s| past 1e100, then NaN): a problem that holds such a row is status 2 and skips the QP.  The timed batch is
    # drawn from the records that stay bounded at the model's and at the true parameters; how many were turned away
    # is part of the line.
    drawn = torch.from_numpy(g[rng.integers(0, g.shape[0], 2 * N * R)]).to(dev)
    tame = torch.ones(2 * N * R, dtype=torch.bool, device=dev)
    for th in (base.expand(2 * N * R, p).contiguous(), true.repeat_interleave(2 * R, dim=0)):
        for lo_ in range(0, 2 * N * R, N * L * R):
            sl = slice(lo_, min(lo_ + N * L * R, 2 * N * R))
            probe, _ = sim.trajectory_jvp(drawn[sl].contiguous(), None, T, 1, None, sel, th[sl].contiguous())
            tame[sl] &= (probe.abs().reshape(probe.shape[0], -1).nan_to_num(nan=float("inf")).amax(dim=1) < 1e3)
    keep = tame.nonzero()[:, 0]
    assert keep.numel() >= N * R, "too few bounded records"
    # (a kept record may land in another problem than it was probed with: what is still not finite is counted below)
    x0 = drawn[keep[:N * R]].contiguous()
    s_obs, _ = sim.trajectory_jvp(x0, None, T, 1, None, sel, true.repeat_interleave(R, dim=0))
    theta = base.expand(N, p).contiguous()
    th_rows = theta.repeat_interleave(R, dim=0)
    V = hb.trajectory_directions(m.input_dim, (), p, device=dev)[None].expand(N * R, -1, -1).contiguous()
    lin = times(lambda: sim.trajectory_jvp(x0, V, T, 1, None, sel, th_rows))
    s, js = sim.trajectory_jvp(x0, V, T, 1, None, sel, th_rows)
    row_start = (torch.arange(N + 1, device=dev) * R).to(torch.int32)
    lam = (1e-4 * torch.tensor((1 / 9, 1 / 3, 1.0, 3.0, 9.0), dtype=torch.float64, device=dev)).expand(N, L).contiguous()
    step = times(lambda: sim.lm_step(row_start, s, s_obs, js, lam, check=False))
    st = sim.lm_step(row_start, s, s_obs, js, lam, check=False)
    cand = (theta[:, None, :] + st["delta"]).reshape(N * L, p).repeat_interleave(R, dim=0)
    x0_c = x0.reshape(N, 1, R, -1).expand(N, L, R, x0.shape[1]).reshape(N * L * R, -1).contiguous()
    obs_c = s_obs.reshape(N, 1, R, T, nsd).expand(N, L, R, T, nsd).reshape(N * L * R, T, nsd).contiguous()
    roll = times(lambda: sim.trajectory_jvp(x0_c, None, T, 1, None, sel, cand))
    s_c, _ = sim.trajectory_jvp(x0_c, None, T, 1, None, sel, cand)
    cand_start = (torch.arange(N * L + 1, device=dev) * R).to(torch.int32)
    price = times(lambda: sim.lm_step(cand_start, s_c, obs_c, None, check=False))
    whole = times(lambda: tds_amd.sysid(sim, x0, s_obs, sel, theta, T, iterations=1))
    res = tds_amd.sysid(sim, x0, s_obs, sel, theta, T, iterations=1)
    parts = [min(lin), min(step), min(roll), min(price)]
    emit({"case": f"one sysid iteration, ant, {N} problems x {R} rows, T={T}, p={p}, L={L}",
          "jacobian_call_ms": rng_ms(lin), "lm_step_ms": rng_ms(step), "candidate_rollout_ms": rng_ms(roll),
          "candidate_costs_ms": rng_ms(price), "sysid_iterations_1_ms": rng_ms(whole),
          "jacobian_share_of_the_four": round(parts[0] / sum(parts), 3),
          "accepted": int((res["pick_trace"] >= 0).sum()), "candidates": N * L,
          "records_drawn": 2 * N * R, "records_turned_away_as_unbounded": int((~tame).sum()),
          "status_1": int((st["status"] == 1).sum()), "status_2": int((st["status"] == 2).sum()),
          "rows_with_a_state_not_finite": int((~torch.isfinite(s)).reshape(N * R, -1).any(dim=1).sum()),
          "rows_with_a_derivative_not_finite": int((~torch.isfinite(js)).reshape(N * R, -1).any(dim=1).sum()),
          "rows_with_an_observation_not_finite": int((~torch.isfinite(s_obs)).reshape(N * R, -1).any(dim=1).sum())})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("# tools/lm_timing.py: warm-up + %d calls each, device-synchronised, one process, profiler off\n" % args.reps)
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
