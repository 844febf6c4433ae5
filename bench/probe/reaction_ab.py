"""Same-process A/B: pcg1 iterations with a reaction field (c = 100 everywhere) against the constant-sigma sweeps
(sigma = 100) -- the same operator, so the same iteration path; the field sweeps read 8 B/pt more per sweep in
fp64 (40 against 32 B/pt plain, 56 against 48 in a w sweep: 136 against 112 B/pt over a w-cycle, 1.21).

    python bench/probe/reaction_ab.py [--n 16384] [--dtype fp64] [--rounds 3] [--iters 192]

Per round the two sessions are built one after the other (the second gets the field block the first released),
pcg1 forced; each is initialised, warmed by 32 iterations, then `iters` graph-replayed iterations are timed between
two synchronisations.  One JSON line per measurement and a summary line (ratio of the round means, and the spread
of the per-round ratios).
"""
import argparse
import importlib
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
pmx = importlib.import_module("poisson-ellipse-openmp-mpi-cuda-new_amd")


def timed(session, iters):
    session.init()
    session.step(32)
    session.synchronize()
    session.prepare(iters)
    t0 = time.perf_counter()
    session.step(iters)
    session.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6, session.path_stats()


def main():
    import torch

    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--dtype", default="fp64")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=192)
    a = ap.parse_args()
    kw = dict(algo="pcg1", block_tiles=0, dtype=a.dtype)
    # the solves must not stop inside the timed region
    base = dict(M=a.n, N=a.n, delta=1e-300, max_iter=10 ** 9)
    c = torch.full((a.n + 1, a.n + 1), 100.0, dtype=torch.float64, device="cuda")
    rows = {"sigma": [], "field": []}
    for rnd in range(a.rounds):
        for name in ("sigma", "field"):
            if name == "sigma":
                s = pmx.make_session(pmx.PoissonEllipse(sigma=100.0, **base), **kw)
            else:
                s = pmx.make_session(pmx.PoissonEllipse(**base), reaction=c, **kw)
            us, path = timed(s, a.iters)
            rows[name].append(us)
            print(json.dumps(dict(round=rnd, variant=name, n=a.n, dtype=a.dtype, us_per_iteration=round(us, 2),
                                  eager_iters=path["eager_iters"], device_bytes=s.device_bytes, tile=s.tile["rows"])),
                  flush=True)
            del s
    ratios = [f / g for f, g in zip(rows["field"], rows["sigma"])]
    mean = sum(rows["field"]) / sum(rows["sigma"])
    print(json.dumps(dict(summary=True, n=a.n, dtype=a.dtype, ratio=round(mean, 4),
                          ratio_min=round(min(ratios), 4), ratio_max=round(max(ratios), 4),
                          sigma_us=[round(v, 2) for v in rows["sigma"]], field_us=[round(v, 2) for v in rows["field"]])))


if __name__ == "__main__":
    main()
