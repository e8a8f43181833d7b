#!/usr/bin/env python3
"""Developer tool (GPU box): what one occupancy sample costs next to the code it would otherwise borrow and next to a step.
Two workloads -- the pitzDaily 1e7-particle cloud as bench.py builds it, and the TJunction 4e6-particle cloud as the tutorial's
dictionary seeds it -- each in a process of its own under its own time limit, one after the other (the second starts only if the
first ended well).  Per workload, device events around 50 back-to-back launches, three repeats with (a) and (b) alternating:
  (a) cpf_occupancy_sample_dev          (b) cpf_cell_histogram_dev on the same array          (c) the step launch (D = 1.5e-5)
on the cloud fresh from a sort, then (a) and (b) once more on the cloud 25 cycles of diffusion past that sort.
  python tools/occupancy_cost.py [--out FILE.jsonl] [--launches 50] [--seconds 240]        prints one JSON line per workload"""
import argparse
import json
import os
import shlex
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
WORKLOADS = (("pitz", 10_000_000), ("tjunction_run", 4_000_000))
D, DT, STALE_CYCLES = 1.5e-5, 1e-4, 25


def worker(a):
    import torch
    from _cases import make_case
    from _spinup import device_spinup
    from cudaparticlesfoam_amd.api import Context
    dev = torch.device("cuda", 0)
    ctx = Context(0); ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    n = a.particles
    mesh, x, y, z, c, _ = make_case(a.worker, ctx, torch, n, dev)
    p = lambda t: t.data_ptr()   # noqa: E731
    ctx.set_option("stats", 0)
    g = torch.arange(n, dtype=torch.int64, device=dev)
    ctx.sort_by_cell_dev(p(x), p(y), p(z), p(c), p(g), n)
    w = torch.zeros(mesh.n_cells, dtype=torch.float64, device=dev)
    device_spinup(ctx, torch, x, y, z, c, n, DT)

    def timed(f):
        """ms per launch: events around a.launches back-to-back launches, after five warm-up launches"""
        for _ in range(5):
            f()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            f()
        e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) / a.launches

    def sample_and_histogram(cell):
        rows = {"occupancy_sample_dev": [], "cell_histogram_dev": []}
        for _ in range(3):
            rows["occupancy_sample_dev"].append(timed(lambda: ctx.occupancy_sample_dev(p(cell), n)))
            rows["cell_histogram_dev"].append(timed(lambda: ctx.cell_histogram_dev(p(cell), n, 1.0, p(w))))
        return {k: dict(ms=round(sorted(v)[1], 5), repeats_ms=[round(t, 5) for t in v]) for k, v in rows.items()}

    out = dict(case=a.worker, particles=n, cells=mesh.n_cells, launches=a.launches, D=D, dt=DT,
               id_bytes=4 * n, id_bound_ms_at_6_TBps=round(4 * n / 6.0e12 * 1e3, 5))
    out["sorted"] = sample_and_histogram(c)
    # the counts agree with the yardstick's on this array (the histogram overwrites, the sample adds: one sample after a reset)
    ctx.occupancy_reset(); ctx.occupancy_sample_dev(p(c), n)
    counts, _ = ctx.occupancy()
    ctx.cell_histogram_dev(p(c), n, 1.0, p(w)); torch.cuda.synchronize()
    out["counts_equal_histogram"] = bool((w.cpu().numpy() == counts.astype("float64")).all())
    # (c) the step launch next to it: single-cycle launches with the kick, from the freshly sorted cloud on (scratch copies)
    sx, sy, sz, sc = x.clone(), y.clone(), z.clone(), c.clone()
    step = [0]

    def one_step():
        ctx.step_dev(p(sx), p(sy), p(sz), p(sc), p(g), None, n, DT, D, step[0], 1, 0); step[0] += 1
    out["step_launch_ms"] = round(timed(one_step), 5)
    out["step_kernel"] = ctx.step_kernel_name(D, 0)
    # ... and on a cloud STALE_CYCLES cycles of diffusion past its last sort
    sx, sy, sz, sc = x.clone(), y.clone(), z.clone(), c.clone()
    ctx.step_dev(p(sx), p(sy), p(sz), p(sc), p(g), None, n, DT, D, 0, STALE_CYCLES, 0)
    out["stale_%d_cycles" % STALE_CYCLES] = sample_and_histogram(sc)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", default=None, help="(internal) run one workload in this process")
    ap.add_argument("--particles", type=int, default=0)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--seconds", type=int, default=240, help="time limit of each workload's process")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.launches < 50:
        ap.error("--launches: at least 50")
    if a.worker:
        return worker(a)
    me = os.path.abspath(__file__)
    steps = []
    for case, n in WORKLOADS:
        cmd = ["timeout", "-k", "10", str(a.seconds), sys.executable, me, "--worker", case, "--particles", str(n),
               "--launches", str(a.launches)] + (["--out", a.out] if a.out else [])
        steps.append(" ".join(shlex.quote(t) for t in cmd))
    sys.exit(subprocess.run(" && ".join(steps), shell=True).returncode)


if __name__ == "__main__":
    main()
