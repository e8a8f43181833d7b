#!/usr/bin/env python3
"""Developer tool (GPU box): what tracer tags (cpf_tag_*; csrc/cpf_tags.hip) cost next to the kernels they ride on.  The pitzDaily
1e7-particle cloud as bench.py seeds it, D = 1.5e-5, sink = the outlet patch's 57 owner cells in two groups (upper / lower half),
source = the inlet's 60 fan triangles weighted by inflow in two origins (upper / lower half), tools/age_cost.py's steady recycling
-- on the CONTEXT-OWNED cloud, the only one the tag entries know.  Its arrays cannot be restored from a copy between launches, so
THREE contexts run the same recycled run in lockstep on one stream: one with tags, one with age tracking (the yardstick the
issue names), one plain.  The runs are bit-identical (the tool checks it): at every cycle all hold the same arrays, and each call
is bracketed by a pair of events.
  cycle = step (1 cycle), sink, respawn of all dead on the source, occupancy sample[, tag sample | age sample]; re-sort every 25.
First 200 cycles to steady recycling, then --periods sort periods are timed.  Per call the median over the timed cycles that are
"fresh" (the first 3 after a sort) and over those that are "stale" (the last 3 before the next):
  sink_plain / sink_tags / sink_ages            cpf_sink_apply: sink_kernel; tag_transfer_kernel + sink_kernel; age_absorb_kernel
  respawn_plain / respawn_tags / respawn_ages   cpf_respawn_source: alone; tag_stamp_kernel first; age_stamp_kernel first
  occupancy / tag_sample / age_sample           the three samples
  step                                          the step launch of the tagged cloud
Then the source is replaced by a table of 4098 triangles (the inlet's, each cut into slivers: past what inlet_place_kernel stages,
and the stamp searches either table in memory) and the same number of periods is timed again ("past_4096").
An event pair round one call carries its launch gaps with it: the figures are call times on a busy stream, not kernel times.
  python tools/tag_cost.py [--out FILE.jsonl] [--periods 4] [--seconds 500]        prints one JSON line"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
D, DT, STEADY_CYCLES, SORT_EVERY, EDGE = 1.5e-5, 1e-4, 200, 25, 3


def worker(a):
    import numpy as np
    import torch
    import bench
    from source_cost import slivers
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

    def halves(t):
        y = t.mean(1)[:, 1]
        return np.where(y > np.median(tri.mean(1)[:, 1]), 2, 1).astype(np.int32)     # origin 0 is the initial cloud

    pieces = -(-4098 // tri.shape[0])
    piece_of = np.repeat(np.arange(tri.shape[0]), pieces)[:4098]
    tables = {"inlet": (tri, weights, depth),
              "past_4096": (slivers(tri, pieces)[:4098], np.repeat(weights / pieces, pieces)[:4098], depth[piece_of])}
    ctxs, xyz = {}, None
    for kind in ("tags", "ages", "plain"):
        ctx = Context(0); ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.set_option("stats", 0); ctx.set_option("sort_interval", SORT_EVERY)
        ctx.set_mesh(mesh); ctx.set_velocity(U)
        if xyz is None:
            x, y, z, _ = bench.seed_in_fluid(ctx, torch, n, pz.DOMAIN_BOX, 1000, dev)
            xyz = torch.stack([x, y, z], 1).cpu().numpy()
            del x, y, z
        ctx.set_particles(xyz); ctx.locate_initial(); ctx.sort_by_cell()
        ctx.set_sink_cells(sink)
        if kind == "tags":
            ctx.tag_enable(3, 2); ctx.set_sink_groups(sink, groups)
        if kind == "ages":
            ctx.age_enable(SORT_EVERY, 64)
        ctxs[kind] = ctx
    tags, ages, plain = ctxs["tags"], ctxs["ages"], ctxs["plain"]

    def set_table(name):
        t, w, d = tables[name]
        for ctx in ctxs.values():
            ctx.set_source_triangles(t, w, d)
        tags.set_source_origins(halves(t))
        return int(tags.source_table()[1].size)

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
        timed("step", group if since else None, lambda: tags.step(DT, D, 1))
        ages.step(DT, D, 1); plain.step(DT, D, 1)
        timed("sink_tags", group, tags.sink_apply)
        timed("sink_ages", group, ages.sink_apply)
        timed("sink_plain", group, plain.sink_apply)
        timed("respawn_tags", group, lambda: tags.respawn_source(-1))
        timed("respawn_ages", group, lambda: ages.respawn_source(-1))
        timed("respawn_plain", group, lambda: plain.respawn_source(-1))
        timed("occupancy", group, tags.occupancy_sample)
        timed("tag_sample", group, tags.tag_sample)
        timed("age_sample", group, ages.age_sample)
        ages.occupancy_sample(); plain.occupancy_sample()

    def summary():
        out = {}
        for group in ("fresh", "stale"):
            g = {}
            for (name, grp), pairs in rows.items():
                if grp == group:
                    ms = sorted(e0.elapsed_time(e1) for e0, e1 in pairs)
                    g[name] = dict(ms=round(ms[len(ms) // 2], 5), min_ms=round(ms[0], 5), max_ms=round(ms[-1], 5), samples=len(ms))
            g["transfer_pass_ms"] = round(g["sink_tags"]["ms"] - g["sink_plain"]["ms"], 5)
            g["transfer_pass_over_plain_sink"] = round(g["transfer_pass_ms"] / g["sink_plain"]["ms"], 3)
            g["tag_stamp_ms"] = round(g["respawn_tags"]["ms"] - g["respawn_plain"]["ms"], 5)
            g["age_stamp_ms"] = round(g["respawn_ages"]["ms"] - g["respawn_plain"]["ms"], 5)
            g["tag_sample_over_occupancy"] = round(g["tag_sample"]["ms"] / g["occupancy"]["ms"], 3)
            g["tag_sample_over_age_sample"] = round(g["tag_sample"]["ms"] / g["age_sample"]["ms"], 3)
            out[group] = g
        rows.clear()
        return out

    out = dict(case="pitz", particles=n, cells=mesh.n_cells, sink_cells=int(sink.size), D=D, dt=DT, periods=a.periods,
               sort_every=SORT_EVERY, steady_cycles=STEADY_CYCLES, origin_table_bytes=n, step_kernel=tags.step_kernel_name(D, 0))
    out["triangles_inlet"] = set_table("inlet")
    for k in range(STEADY_CYCLES):
        cycle(k, False)
    torch.cuda.synchronize()
    out["absorbed_per_cycle"] = tags.recycle_counts()["absorbed"] / STEADY_CYCLES
    tags.tag_reset()
    k0 = STEADY_CYCLES
    for k in range(k0, k0 + a.periods * SORT_EVERY):
        cycle(k, True)
    torch.cuda.synchronize()
    out["inlet"] = summary()
    out["triangles_past_4096"] = set_table("past_4096")
    k0 += a.periods * SORT_EVERY
    for k in range(k0, k0 + SORT_EVERY):                            # one period for the new table's respawns to reach the cloud
        cycle(k, False)
    k0 += SORT_EVERY
    for k in range(k0, k0 + a.periods * SORT_EVERY):
        cycle(k, True)
    torch.cuda.synchronize()
    out["past_4096"] = summary()
    for group in ("fresh", "stale"):
        out["past_4096"][group]["tag_stamp_over_inlet"] = round(out["past_4096"][group]["tag_stamp_ms"] /
                                                                out["inlet"][group]["tag_stamp_ms"], 3)
    # the three runs are one run: neither tags nor ages changed anything of the cloud
    p_ = [c.get_particles() for c in (tags, ages, plain)]
    out["runs_identical"] = bool(all(np.array_equal(p_[0][0].view(np.int64), q[0].view(np.int64)) and np.array_equal(p_[0][1], q[1])
                                     for q in p_[1:]) and tags.recycle_counts() == ages.recycle_counts() == plain.recycle_counts())
    T = tags.transfer()
    f, ns = tags.tag_field()
    out["transfer"] = T.tolist(); out["tag_samples"] = int(ns)
    out["field_sums_per_origin"] = [int(v) for v in f.sum(1)]
    out["origins_in_cloud"] = [int(v) for v in np.bincount(tags.tag_origins(), minlength=3)]
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
    ap.add_argument("--periods", type=int, default=4, help="sort periods of 25 cycles that are timed, per table")
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
