#!/usr/bin/env python3
"""Developer tool (GPU box): what it costs to let the patch source follow the velocity field (cpf_source_follow;
csrc/cpf_inflow.hip), in one process under its own time limit.  The pitzDaily mesh, a field on the device, three contexts on one
stream:
  follow off        cpf_set_velocity_dev alone -- the field's layout, what every Eulerian step pays anyway;
  follow on, 60     the same call with the inlet patch's 60 fan triangles following: one fused launch more;
  follow on, 65536  the same with a synthetic source of 2^16 triangles (the inlet's, cut into slivers): the four launches.
A figure is `calls` calls back to back between two device events, after 20 warm-up calls, per call; the median of three such
windows with the three listed (their spread is the run-to-run spread); the three contexts alternate within a repeat.  Then today's
route, the baseline the feature replaces: per step ``inflow_weights`` in numpy and ``set_source_triangles`` (table on the host, a
wait for the stream, two allocations, two blocking copies) behind the same cpf_set_velocity_dev, timed on the host clock around a
device synchronise, per step over `steps` steps.
  python tools/inflow_cost.py [--out FILE.jsonl] [--calls 2000] [--steps 50] [--seconds 300]        prints one JSON line"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
DT = 1e-4


def worker(a):
    import torch
    from source_cost import slivers
    from cudaparticlesfoam_amd import api
    from cudaparticlesfoam_amd.cases import pitzdaily as pz
    dev = torch.device("cuda", 0)
    mesh = pz.pitzdaily_mesh()
    U = pz.analytic_step_u(mesh)
    tU = torch.from_numpy(np.ascontiguousarray(U)).to(dev)
    tri, of = mesh.face_triangles(mesh.patch_faces("inlet"))
    cells = mesh.owner[of].astype(np.int32)
    pieces = -(-65536 // tri.shape[0])
    cut = slivers(tri, pieces)[:65536]
    cut_cells = np.repeat(cells, pieces)[:65536]
    stream = torch.cuda.current_stream().cuda_stream

    def context(triangles, owner):
        ctx = api.Context(0); ctx.set_stream(stream)
        ctx.set_option("stats", 0)
        ctx.set_mesh(mesh)
        if triangles is not None:
            ctx.set_source_triangles(triangles, None, (0.0, 0.0))
            ctx.source_follow(owner, DT)
        return ctx

    ctxs = {"follow_off": context(None, None), "follow_on_60": context(tri, cells), "follow_on_65536": context(cut, cut_cells)}
    torch.cuda.synchronize()

    def window(ctx):
        for _ in range(20):
            ctx.set_velocity_dev(tU.data_ptr(), mesh.n_cells)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            ctx.set_velocity_dev(tU.data_ptr(), mesh.n_cells)
        e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) / a.calls

    rows = {name: [] for name in ctxs}
    for _ in range(3):
        for name, ctx in ctxs.items():
            rows[name].append(window(ctx))
    out = dict(case="pitz", cells=mesh.n_cells, calls=a.calls, steps=a.steps,
               triangles={name: int(ctx.source_table()[1].size) for name, ctx in ctxs.items()},
               counts={name: ctx.source_follow_counts() for name, ctx in ctxs.items()})
    for name, v in rows.items():
        out[name] = dict(ms=round(sorted(v)[1], 5), repeats_ms=[round(t, 5) for t in v])
    for name in ("follow_on_60", "follow_on_65536"):
        out[name]["extra_ms"] = round(out[name]["ms"] - out["follow_off"]["ms"], 5)
    # today's route on a context of its own: weights in numpy, a new table per step
    ctx = context(tri, cells); ctx.source_unfollow()
    per_step = []
    for rep in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            ctx.set_velocity_dev(tU.data_ptr(), mesh.n_cells)
            w = api.inflow_weights(mesh, U, tri, of)
            ctx.set_source_triangles(tri, w, (0.0, 0.0))
        torch.cuda.synchronize()
        per_step.append((time.perf_counter() - t0) * 1e3 / a.steps)
    out["todays_route_60"] = dict(ms=round(sorted(per_step)[1], 5), repeats_ms=[round(t, 5) for t in per_step], clock="host")
    # the same steps with following on, on the same clock
    ctx = ctxs["follow_on_60"]
    per_step = []
    for rep in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            ctx.set_velocity_dev(tU.data_ptr(), mesh.n_cells)
        torch.cuda.synchronize()
        per_step.append((time.perf_counter() - t0) * 1e3 / a.steps)
    out["follow_on_60_host_clock"] = dict(ms=round(sorted(per_step)[1], 5), repeats_ms=[round(t, 5) for t in per_step], clock="host")
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    for c in list(ctxs.values()):
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true", help="(internal) run the workload in this process")
    ap.add_argument("--calls", type=int, default=2000)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--seconds", type=int, default=300, help="time limit of the workload's process")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    cmd = ["timeout", "-k", "10", str(a.seconds), sys.executable, os.path.abspath(__file__), "--worker", "--calls", str(a.calls),
           "--steps", str(a.steps)] + (["--out", a.out] if a.out else [])
    sys.exit(subprocess.run(cmd).returncode)


if __name__ == "__main__":
    main()
