#!/usr/bin/env python3
"""Developer tool (GPU box): what routes (cpf_route_*; csrc/cpf_routes.hip) cost next to the two-pass path they replace.  The
pitzDaily 1e7-particle cloud as bench.py seeds it, D = 1.5e-5, sink = the outlet patch's 57 owner cells in two groups (upper /
lower half), source = the inlet's 60 fan triangles weighted by inflow in two origins (upper / lower half), tools/tag_cost.py's
steady recycling on the CONTEXT-OWNED cloud.  FOUR contexts run the same recycled run in lockstep on one stream, all with tags
and age tracking on:
  routes      routes on, 16 residence-time bins: the joint histogram 2 x 2 x 16 is staged in LDS
  twin        routes off, 16 bins: cpf_sink_apply is tag_transfer_kernel + age_absorb_kernel, the path of before
  routes_big  routes on, 4096 bins: the joint histogram 2 x 2 x 4096 is added to in global memory
  twin_big    routes off, 4096 bins
The runs are bit-identical (the tool checks it): at every cycle all hold the same arrays, and each call is bracketed by a pair of
events.
  cycle = step (1 cycle), sink, respawn of all dead on the source, samples; re-sort every 25.
First 200 cycles to steady recycling, then --periods sort periods are timed.  Per call the median, minimum and maximum over the
timed cycles that are "fresh" (the first 3 after a sort) and over those that are "stale" (the last 3 before the next):
  sink_routes / sink_twin / sink_routes_big / sink_twin_big     cpf_sink_apply
  route_sample / age_sample / tag_sample                        the three field samples, on `routes`' cloud
(a) fused_over_twin = sink_routes / sink_twin, and not_slower: the fused call's median is within the twin's own min-max spread
    above the twin's median -- the resolution of the comparison.  The same for the 4096-bin pair, and staged against global.
(b) route_sample over age_sample and over tag_sample.
An event pair round one call carries its launch gaps with it: the figures are call times on a busy stream, not kernel times.
  python tools/route_cost.py [--out FILE.jsonl] [--periods 4] [--seconds 500]        prints one JSON line"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
D, DT, STEADY_CYCLES, SORT_EVERY, EDGE = 1.5e-5, 1e-4, 200, 25, 3
KINDS = {"routes": (16, True), "twin": (16, False), "routes_big": (4096, True), "twin_big": (4096, False)}      # bins, routes on


def worker(a):
    import numpy as np
    import torch
    import bench
    from cudaparticlesfoam_amd import api
    from cudaparticlesfoam_amd.api import Context
    from cudaparticlesfoam_amd.cases import pitzdaily as pz
    from cudaparticlesfoam_amd.parallel import x_slab_renumbering
    dev = torch.device("cuda", 0)
    n = a.particles
    mesh0 = pz.pitzdaily_mesh(); c0, _ = mesh0.cell_centres_volumes()
    mesh = mesh0.renumber_cells(x_slab_renumbering(c0))
    centres, _ = mesh.cell_centres_volumes()
    U = pz.uniform_u(mesh)
    sink = mesh.patch_cells("outlet")
    groups = (centres[sink, 1] > np.median(centres[sink, 1])).astype(np.int32)
    tri, of = mesh.face_triangles(mesh.patch_faces("inlet"))
    weights = api.inflow_weights(mesh, U, tri, of)
    un = weights / (0.5 * np.linalg.norm(np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]), axis=1))
    depth = np.stack([np.zeros(un.size), un * DT], 1)
    y = tri.mean(1)[:, 1]
    origins = (y > np.median(y)).astype(np.int32)
    ctxs, xyz = {}, None
    for kind, (bins, routed) in KINDS.items():
        ctx = Context(0); ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.set_option("stats", 0); ctx.set_option("sort_interval", SORT_EVERY)
        ctx.set_mesh(mesh); ctx.set_velocity(U)
        if xyz is None:
            x, y_, z, _ = bench.seed_in_fluid(ctx, torch, n, pz.DOMAIN_BOX, 1000, dev)
            xyz = torch.stack([x, y_, z], 1).cpu().numpy()
            del x, y_, z
        ctx.set_source_triangles(tri, weights, depth)
        ctx.set_particles(xyz); ctx.locate_initial(); ctx.sort_by_cell()
        ctx.age_enable(SORT_EVERY, bins)
        ctx.tag_enable(2, 2); ctx.set_sink_groups(sink, groups); ctx.set_source_origins(origins)
        if routed:
            ctx.route_enable()
        ctxs[kind] = ctx
    routes = ctxs["routes"]
    rows = {}

    def timed(name, group, f):
        if group is None:
            return f()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); f(); e1.record()
        rows.setdefault((name, group), []).append((e0, e1))

    def cycle(k, timing):
        since = (k + 1) % SORT_EVERY                                # cycles since a sort, behind this cycle's step (0: it ended in one)
        group = None if not timing else "fresh" if since < EDGE else "stale" if since >= SORT_EVERY - EDGE else None
        for ctx in ctxs.values():
            ctx.step(DT, D, 1)
        for kind, ctx in ctxs.items():
            timed("sink_" + kind, group, ctx.sink_apply)
        for ctx in ctxs.values():
            ctx.respawn_source(-1)
        timed("route_sample", group, routes.route_sample)
        timed("age_sample", group, routes.age_sample)
        timed("tag_sample", group, routes.tag_sample)

    def summary():
        out = {}
        for group in ("fresh", "stale"):
            g = {}
            for (name, grp), pairs in rows.items():
                if grp == group:
                    ms = sorted(e0.elapsed_time(e1) for e0, e1 in pairs)
                    g[name] = dict(ms=round(ms[len(ms) // 2], 5), min_ms=round(ms[0], 5), max_ms=round(ms[-1], 5), samples=len(ms))
            for fused, twin, tag in (("sink_routes", "sink_twin", ""), ("sink_routes_big", "sink_twin_big", "_big")):
                spread = g[twin]["max_ms"] - g[twin]["min_ms"]
                g["fused_over_twin" + tag] = round(g[fused]["ms"] / g[twin]["ms"], 3)
                g["twin_spread_ms" + tag] = round(spread, 5)
                g["not_slower" + tag] = bool(g[fused]["ms"] <= g[twin]["ms"] + spread)
            g["global_over_staged"] = round(g["sink_routes_big"]["ms"] / g["sink_routes"]["ms"], 3)
            g["route_sample_over_age_sample"] = round(g["route_sample"]["ms"] / g["age_sample"]["ms"], 3)
            g["route_sample_over_tag_sample"] = round(g["route_sample"]["ms"] / g["tag_sample"]["ms"], 3)
            out[group] = g
        rows.clear()
        return out

    out = dict(case="pitz", particles=n, cells=mesh.n_cells, sink_cells=int(sink.size), triangles=int(tri.shape[0]), D=D, dt=DT,
               periods=a.periods, sort_every=SORT_EVERY, steady_cycles=STEADY_CYCLES, step_kernel=routes.step_kernel_name(D, 0))
    for k in range(STEADY_CYCLES):
        cycle(k, False)
    torch.cuda.synchronize()
    out["absorbed_per_cycle"] = routes.recycle_counts()["absorbed"] / STEADY_CYCLES
    for ctx in ctxs.values():
        ctx.age_reset(); ctx.tag_reset()
    for kind, (_, routed) in KINDS.items():
        if routed:
            ctxs[kind].route_reset()
    k0 = STEADY_CYCLES
    for k in range(k0, k0 + a.periods * SORT_EVERY):
        cycle(k, True)
    torch.cuda.synchronize()
    out.update(summary())
    # the four runs are one run, and what age and tags report does not know of routes
    p_ = [c.get_particles() for c in ctxs.values()]
    same = all(np.array_equal(p_[0][0].view(np.int64), q[0].view(np.int64)) and np.array_equal(p_[0][1], q[1]) for q in p_[1:])
    same = same and all(c.recycle_counts() == routes.recycle_counts() and np.array_equal(c.transfer(), routes.transfer())
                        for c in ctxs.values())
    same = same and np.array_equal(routes.age_histogram(), ctxs["twin"].age_histogram())
    same = same and np.array_equal(ctxs["routes_big"].age_histogram(), ctxs["twin_big"].age_histogram())
    out["runs_identical"] = bool(same)
    for kind in ("routes", "routes_big"):
        h = ctxs[kind].route_histogram()
        out["marginals_hold_" + kind] = bool(np.array_equal(h.sum(2), ctxs[kind].transfer()) and
                                             np.array_equal(h.sum((0, 1)), ctxs[kind].age_histogram()))
    out["transfer"] = routes.transfer().tolist()
    s, c, ns = routes.route_field()
    out["route_samples"] = int(ns)
    out["field_counts_are_tag_field"] = bool(np.array_equal(c, routes.tag_field()[0].T))
    out["field_sums_are_age_field"] = bool(np.array_equal(s.sum(1), routes.age_field()[0]))
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(line + "\n")
    for c in ctxs.values():
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true", help="(internal) run the workload in this process")
    ap.add_argument("--particles", type=int, default=10_000_000)
    ap.add_argument("--periods", type=int, default=4, help="sort periods of 25 cycles that are timed")
    ap.add_argument("--seconds", type=int, default=500, help="time limit of the workload's process")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.periods < 2:
        ap.error("--periods: at least 2")
    if a.worker:
        return worker(a)
    cmd = ["timeout", "-k", "10", str(a.seconds), sys.executable, os.path.abspath(__file__), "--worker", "--particles", str(a.particles),
           "--periods", str(a.periods)] + (["--out", a.out] if a.out else [])
    sys.exit(subprocess.run(cmd).returncode)


if __name__ == "__main__":
    main()
