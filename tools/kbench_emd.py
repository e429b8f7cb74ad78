"""Kernel bench of the earth mover's distance (shapeformer_amd/metrics.py emd_dev, csrc/emd.hip).

    python tools/kbench_emd.py [--out profiles/NAME.txt] [--quick] [--chunks]

One JSON line per case: one pair at n = 512 / 2048 / 8192, 256 and 4096 pairs at 2048 (pairs over two collections of 64 clouds), with
rounds, ms (the whole call: launches and the read-back of the unfinished counter per launch), pairs per second, the share of the
workgroups' time in rounds with fewer than 16 bidders (the device's own clock, emd_dev(ticks=True), in a run of its own), and the host route (copy to the
host, float64 cost matrix, scipy.optimize.linear_sum_assignment) at the sizes where that finishes; then a 32 x 32 set_metrics under
both metrics.  --chunks adds the sweep of chunk_rounds behind the default.  Clouds are jittered spheres, as in the tests.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from shapeformer_amd import metrics as M  # noqa: E402


def shell(n, seed, r=0.5, jitter=0.01):
    rs = np.random.RandomState(seed)
    u = rs.randn(n, 3)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    return (u * r + rs.randn(n, 3) * jitter).astype(np.float32)


def timed(fn, reps):
    fn()                                                           # warm-up: library load, LDS attribute, allocator
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return out, float(np.median(ts))


def host_route(a, b):
    from scipy.optimize import linear_sum_assignment
    t = time.perf_counter()
    A, B = a.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)
    C = np.sqrt(((A[:, None, :] - B[None, :, :]) ** 2).sum(-1))
    r, c = linear_sum_assignment(C)
    return float(C[r, c].mean()), (time.perf_counter() - t) * 1e3


def case(name, X, Y, pairs, dev, reps, host, **kw):
    n = X.shape[1]
    _, ms = timed(lambda: M.emd_dev(X, Y, pairs=pairs, **kw), reps)
    e, d = M.emd_dev(X, Y, pairs=pairs, details=True, ticks=True, **kw)      # the clock reads cost time: a run of their own
    tk = d["ticks"].cpu().numpy().astype(np.float64)
    rounds = d["rounds"].cpu().numpy()
    row = {"kernel": "emd_dev", "case": name, "pairs": len(pairs), "n": n, "ms": ms, "pairs_per_s": len(pairs) / ms * 1e3,
           "rounds_mean": float(rounds.mean()), "rounds_max": int(rounds.max()), "rounds_over_n_max": float(rounds.max()) / n,
           "status_nonzero": int((d["status"] != 0).sum()), "emd_mean": float(e.mean()),
           "share_of_time_below_16_bidders": float(tk[:, 0].sum() / max(tk[:, 1].sum(), 1.0)),
           "workgroup_ms_max": float(tk[:, 1].max() / 1e5), **{k: v for k, v in kw.items()}}
    if host:
        i, j = pairs[0]
        opt, hms = host_route(X[i], Y[j])
        row.update(host_ms_per_pair=hms, host_emd=opt, emd_minus_host=float(e[0]) - opt, eps_final=float(d["eps_final"][0]),
                   x_host_per_pair=hms / (ms / len(pairs)))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true", help="skip the 4096-pair case, n = 8192 and the 32 x 32 matrices")
    ap.add_argument("--chunks", action="store_true", help="sweep chunk_rounds at n = 2048")
    args = ap.parse_args()
    dev = torch.device("cuda")
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    one = np.array([[0, 0]])
    for n in (512, 2048) if args.quick else (512, 2048, 8192):
        X = torch.from_numpy(np.stack([shell(n, 1)])).to(dev)
        Y = torch.from_numpy(np.stack([shell(n, 2)])).to(dev)
        emit(case(f"1 x {n}", X, Y, one, dev, 5, host=n <= 2048))
    X = torch.from_numpy(np.stack([shell(2048, 10 + i) for i in range(64)])).to(dev)
    Y = torch.from_numpy(np.stack([shell(2048, 100 + i) for i in range(64)])).to(dev)
    grid = np.stack(np.divmod(np.arange(4096), 64), 1)
    for P in (256,) if args.quick else (256, 4096):
        emit(case(f"{P} x 2048", X, Y, grid[:P], dev, 3 if P == 256 else 1, host=False))
    if args.chunks:
        for chunk in (256, 1024, 4096, 16384, 1 << 20):
            emit(case("1 x 2048", X, Y, one, dev, 5, host=False, chunk_rounds=chunk))
            emit(case("256 x 2048", X, Y, grid[:256], dev, 3, host=False, chunk_rounds=chunk))
    if not args.quick:
        G, Rf = X[:32], Y[:32]
        for metric in ("cd", "emd"):
            out, ms = timed(lambda: M.set_metrics(G, Rf, metric=metric), 1)
            emit({"kernel": "set_metrics", "case": "32 x 32 x 2048", "metric": metric, "ms": ms, "pairs": 32 * 32 + 2 * 496,
                  "mmd": out["mmd"], "cov": out["cov"], "1nna": out["1nna"]})
    if args.out:
        with open(args.out, "w") as f:
            for row in rows:
                f.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
