#!/usr/bin/env python3
"""Developer tool (GPU box): what a respawn on the patch source (cpf_respawn_source_dev; csrc/cpf_inlet.hip) costs next to the box
respawn (cpf_respawn_box_dev; csrc/cpf_recycle.hip) on the same arrays, in one process under its own time limit.  The pitzDaily
1e7-particle cloud as bench.py builds it, D = 1.5e-5, sink = the outlet patch's owner cells, source = the 60 fan triangles of the
inlet patch, weighted by inflow, depth 0 .. |U.n| * dt; the box = tools/recycle_cost.py's, the inlet end of the domain.  The
cloud is sorted by cell, and three regimes are timed for both (DESIGN.md 5.7 reports them for the box):
  nobody dead / 1 % of the cloud dead in a run at the tail (where a sort leaves them) / 1 % dead scattered over the array.
The cell array is restored from a copy before every launch; a figure is 50 x (restore, launch) back to back minus 50 x restore
back to back, after five warm-up launches, the median of three such differences, with the three differences listed (their spread
is the run-to-run spread).  Box and source alternate within a regime.  Then the source alone once more with a table of 4098
triangles (the inlet's, each cut into slivers): bounds past the 4096 the kernel stages in LDS, searched in global memory.
  python tools/source_cost.py [--out FILE.jsonl] [--launches 50] [--seconds 400]        prints one JSON line"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
D, DT = 1.5e-5, 1e-4


def slivers(tri, pieces):
    """every triangle (A, B, C) cut into `pieces` triangles (A, B + (C - B) j / pieces, B + (C - B) (j + 1) / pieces)"""
    a, b, c = tri[:, None, 0], tri[:, None, 1], tri[:, None, 2]
    s = np.arange(pieces + 1)[None, :, None] / pieces
    on_bc = b + (c - b) * s
    out = np.stack([np.broadcast_to(a, on_bc[:, :-1].shape), on_bc[:, :-1], on_bc[:, 1:]], 2)
    return np.ascontiguousarray(out.reshape(-1, 3, 3))


def worker(a):
    import torch
    from _cases import make_case
    from _spinup import device_spinup
    from cudaparticlesfoam_amd import api
    from cudaparticlesfoam_amd.cases import pitzdaily as pz
    dev = torch.device("cuda", 0)
    ctx = api.Context(0); ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    n = a.particles
    mesh, x, y, z, c, fields = make_case("pitz", ctx, torch, n, dev)
    U = fields["uniform"]
    p = lambda t: t.data_ptr()   # noqa: E731
    ctx.set_option("stats", 0)
    g = torch.arange(n, dtype=torch.int64, device=dev)
    ctx.set_sink_cells(mesh.patch_cells("outlet"))
    tri, of = mesh.face_triangles(mesh.patch_faces("inlet"))
    weights = api.inflow_weights(mesh, U, tri, of)
    un = weights / (0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1))
    depth = np.stack([np.zeros(un.size), un * DT], 1)
    (lx, ly, lz), (hx, hy, hz) = pz.DOMAIN_BOX
    box = ((lx, ly, lz), (lx + 0.05 * (hx - lx), hy, hz))
    ctx.sort_by_cell_dev(p(x), p(y), p(z), p(c), p(g), n)
    device_spinup(ctx, torch, x, y, z, c, n, DT)
    ctx.step_dev(p(x), p(y), p(z), p(c), p(g), None, n, DT, D, 0, 25, 0)
    ctx.sink_apply_dev(p(c), n)
    ctx.sort_by_cell_dev(p(x), p(y), p(z), p(c), p(g), n)
    torch.cuda.synchronize()

    def timed(f):
        for _ in range(5):
            f()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            f()
        e1.record(); e1.synchronize()
        return e0.elapsed_time(e1) / a.launches

    sx, sy, sz, sc = x.clone(), y.clone(), z.clone(), c.clone()
    live = torch.clamp(c, min=0)
    n_dead = n // 100
    tail = live.clone(); tail[n - n_dead:] = -1
    scattered = live.clone(); scattered[torch.randperm(n, device=dev)[:n_dead]] = -1
    regimes = {"nobody_dead": live, "1pct_dead_in_a_run": tail, "1pct_dead_scattered": scattered}
    epoch = [0]

    def box_call():
        ctx.respawn_box_dev(p(sx), p(sy), p(sz), p(sc), p(g), n, box[0], box[1], -1, epoch[0]); epoch[0] += 1

    def source_call():
        ctx.respawn_source_dev(p(sx), p(sy), p(sz), p(sc), p(g), n, -1, epoch[0]); epoch[0] += 1

    def compare(calls):
        """{regime: {name: {ms, repeats_ms}}}: the calls alternate within a repeat"""
        out = {}
        for regime, cells in regimes.items():
            restore = lambda: sc.copy_(cells)   # noqa: E731
            rows = {name: [] for name in calls}
            for _ in range(3):
                for name, f in calls.items():
                    both = lambda: (restore(), f())   # noqa: E731
                    rows[name].append(timed(both) - timed(restore))
            out[regime] = {name: dict(ms=round(sorted(v)[1], 5), repeats_ms=[round(t, 5) for t in v]) for name, v in rows.items()}
        return out

    out = dict(case="pitz", particles=n, cells=mesh.n_cells, launches=a.launches, D=D, dt=DT, dead=n_dead)
    ctx.set_source_triangles(tri, weights, depth)
    out["triangles"] = int(ctx.source_table()[1].size)
    before = ctx.recycle_counts()
    out["inlet"] = compare({"respawn_box": box_call, "respawn_source": source_call})
    after = ctx.recycle_counts()
    out["drawn"], out["placed"] = after["drawn"] - before["drawn"], after["placed"] - before["placed"]
    for regime, r in out["inlet"].items():
        r["source_over_box"] = round(r["respawn_source"]["ms"] / r["respawn_box"]["ms"], 3)
        r["box_spread_ms"] = round(max(r["respawn_box"]["repeats_ms"]) - min(r["respawn_box"]["repeats_ms"]), 5)
    pieces = -(-4098 // tri.shape[0])
    cut = slivers(tri, pieces)[:4098]
    k = np.repeat(np.arange(tri.shape[0]), pieces)[:4098]
    ctx.set_source_triangles(cut, np.repeat(weights / pieces, pieces)[:4098], depth[k])
    out["triangles_past_lds"] = int(ctx.source_table()[1].size)
    out["past_lds"] = compare({"respawn_source": source_call})
    for regime, r in out["past_lds"].items():
        r["over_staged"] = round(r["respawn_source"]["ms"] / out["inlet"][regime]["respawn_source"]["ms"], 3)
        r["source_over_box"] = round(r["respawn_source"]["ms"] / out["inlet"][regime]["respawn_box"]["ms"], 3)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true", help="(internal) run the workload in this process")
    ap.add_argument("--particles", type=int, default=10_000_000)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--seconds", type=int, default=400, help="time limit of the workload's process")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.launches < 50:
        ap.error("--launches: at least 50")
    if a.worker:
        return worker(a)
    cmd = ["timeout", "-k", "10", str(a.seconds), sys.executable, os.path.abspath(__file__), "--worker", "--particles", str(a.particles),
           "--launches", str(a.launches)] + (["--out", a.out] if a.out else [])
    sys.exit(subprocess.run(cmd).returncode)


if __name__ == "__main__":
    main()
