#!/usr/bin/env python3
"""Host-array against device-tensor data movement of a session, in one process (the `device_io` study
of the bench directory's study runner).  Per storage type, the median wall time of --reps calls, each
fenced by a device synchronisation on both sides:

    init_numpy   Session.init(rhs, w0) with NumPy arrays (host rounding + two pageable uploads)
    init_device  the same with float64 tensors on the device (finite check + scatter kernels)
    gather_numpy Session.gather_local_w() (up to three field downloads + host passes)
    gather_device Session.w_tensor(out=) (gather kernel)
    copy_in / copy_out  torch dst.copy_(src) between an (M+1)x(N+1) tensor and a pitched view of that
                 shape: the bandwidth yardstick of the scatter and gather kernels

Prints one JSON line.
"""
from __future__ import annotations

import argparse
import importlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
PKG = "poisson-ellipse-openmp-mpi-cuda-new_amd"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--M", type=int, default=4096)
    ap.add_argument("--N", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--dtypes", default="fp64,fp32")
    ap.add_argument("--ranks", type=int, default=1)
    ap.add_argument("--algo", default="auto", help="auto, pcg1, pcg2 or ca (pcg1 / pcg2 leave w steps pending)")
    ap.add_argument("--iters", type=int, default=10, help="iterations before the gathers (pending w steps)")
    a = ap.parse_args()

    import numpy as np
    import torch

    pkg = importlib.import_module(PKG)
    dev = torch.device("cuda", 0)
    shape = (a.M + 1, a.N + 1)
    rng = np.random.default_rng(1)
    f, w0 = rng.standard_normal(shape), 1e-3 * rng.standard_normal(shape)
    f_dev, w0_dev = torch.from_numpy(f).to(dev), torch.from_numpy(w0).to(dev)
    out = torch.empty(shape, dtype=torch.float64, device=dev)
    pitch = (a.N + 1 + 63) // 64 * 64 + 64
    pitched = torch.zeros(a.M + 1, pitch, dtype=torch.float64, device=dev)[:, 1:a.N + 2]

    def median_ms(fn, fence):
        t = []
        for _ in range(a.reps + 1):  # the first call warms up
            fence()
            t0 = time.perf_counter()
            fn()
            fence()
            t.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(t[1:])

    res = {"M": a.M, "N": a.N, "reps": a.reps, "ranks": a.ranks, "algo": a.algo, "ms": {}}
    for dt in a.dtypes.split(","):
        s = pkg.make_session(pkg.PoissonEllipse(M=a.M, N=a.N), ranks=a.ranks, dtype=dt, algo=a.algo)

        def fence():
            s.synchronize()
            torch.cuda.synchronize(dev)

        r = {}
        r["init_numpy"] = median_ms(lambda: s.init(rhs=f, w0=w0), fence)
        r["init_device"] = median_ms(lambda: s.init(rhs=f_dev, w0=w0_dev), fence)
        s.init(rhs=f_dev, w0=w0_dev)
        s.step(a.iters)
        st = s.state(0)
        r["pending"] = [st["w_pend_n"], st["w_pend"]]
        r["gather_numpy"] = median_ms(lambda: s.gather_local_w(), fence)
        r["gather_device"] = median_ms(lambda: s.w_tensor(out=out), fence)
        assert np.array_equal(out.cpu().numpy(), s.gather_local_w())
        res["ms"][dt] = r
        del s
    sync = lambda: torch.cuda.synchronize(dev)  # noqa: E731
    res["ms"]["copy_in"] = median_ms(lambda: pitched.copy_(f_dev), sync)
    res["ms"]["copy_out"] = median_ms(lambda: out.copy_(pitched), sync)
    res["gb"] = 2 * 8 * shape[0] * shape[1] / 1e9  # read + write of one fp64 copy
    print(json.dumps(res))


if __name__ == "__main__":
    main()
