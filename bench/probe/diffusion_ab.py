"""Same-process A/B: pcg1 iterations with a diffusion field (k = 1 everywhere, next to c = 100) against the
reaction-field sweeps (c = 100) -- the same operator, so the same iteration path; the diffusion sweeps read the two
face-coefficient fields on top, 16 B/pt more per sweep in fp64 (56 against 40 B/pt plain, 72 against 56 in a w
sweep: 184 against 136 B/pt over a w-cycle, 1.35).

    python bench/probe/diffusion_ab.py [--n 16384] [--dtype fp64] [--rounds 3] [--iters 192]

Per round the two sessions are built one after the other (the second gets the field block the first released),
pcg1 forced; each is initialised, warmed by 32 iterations, then `iters` graph-replayed iterations are timed between
two synchronisations.  One JSON line per measurement and a summary line (ratio of the round means, and the spread
of the per-round ratios).  A study, not a test.
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
    p = pmx.PoissonEllipse(M=a.n, N=a.n, delta=1e-300, max_iter=10 ** 9)
    c = torch.full((a.n + 1, a.n + 1), 100.0, dtype=torch.float64, device="cuda")
    k = torch.ones((a.n + 1, a.n + 1), dtype=torch.float64, device="cuda")
    rows = {"reaction": [], "diffusion": []}
    for rnd in range(a.rounds):
        for name in ("reaction", "diffusion"):
            s = pmx.make_session(p, reaction=c, **(dict(diffusion=k) if name == "diffusion" else {}), **kw)
            us, path = timed(s, a.iters)
            rows[name].append(us)
            print(json.dumps(dict(round=rnd, variant=name, n=a.n, dtype=a.dtype, us_per_iteration=round(us, 2),
                                  eager_iters=path["eager_iters"], device_bytes=s.device_bytes, tile=s.tile["rows"])),
                  flush=True)
            del s
    ratios = [f / g for f, g in zip(rows["diffusion"], rows["reaction"])]
    mean = sum(rows["diffusion"]) / sum(rows["reaction"])
    print(json.dumps(dict(summary=True, n=a.n, dtype=a.dtype, ratio=round(mean, 4),
                          ratio_min=round(min(ratios), 4), ratio_max=round(max(ratios), 4),
                          reaction_us=[round(v, 2) for v in rows["reaction"]],
                          diffusion_us=[round(v, 2) for v in rows["diffusion"]])))


if __name__ == "__main__":
    main()
