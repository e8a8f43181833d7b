#!/usr/bin/env python3
"""Developer tool (GPU box): what zones (cpf_zone_*; csrc/cpf_zones.hip) cost next to the kernels they ride on.  The pitzDaily
1e7-particle cloud as bench.py seeds it, D = 1.5e-5, sink = the outlet patch's owner cells, source = the inlet end of the domain
box: tools/exposure_cost.py's regime and its method -- FOUR contexts run the same recycled run in lockstep on one stream (the runs
are bit-identical: the tool checks it), so at every cycle all hold the same arrays, and each call is bracketed by a pair of events:
  slab4   zones with a map of 4 slabs along x, and age tracking (for the age sample next to it)
  slab63  zones with a map of 63 slabs along x
  dense   exposure with a positive rate in every cell, no zones: the dense accumulate next to the sample
  off     no zones, age tracking: the twin of `slab4`
  cycle = step (1 cycle), zone sample / accumulate, sink, respawn of all dead, occupancy sample, age sample; every cloud re-sorts
  every 25 cycles.
First 200 cycles to steady recycling, then --periods sort periods are timed.  Per call the median, minimum and maximum over the
timed cycles that are "fresh" (the first 3 after a sort) and over those that are "stale" (the last 3 before the next):
  sample_4 / sample_63               cpf_zone_sample of the two maps
  accumulate_dense                   cpf_exposure_accumulate of `dense`
  age_sample / occupancy / step      cpf_age_sample, cpf_occupancy_sample and the step launch of `slab4`: the neighbours
  sink_zoned / sink_twin             cpf_sink_apply of `slab4` (the leave pass, then the age pass) and of `off` (the age pass)
  respawn_stamp / respawn_twin       cpf_respawn_box of `slab4` (age's stamp, the zone stamp, the respawn) and of `off`
An event pair round one launch carries the launch gap with it: the figures are call times on a busy stream, not kernel times.
  python tools/zones_cost.py [--out FILE.jsonl] [--periods 8] [--seconds 400]        prints one JSON line"""
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
    from cudaparticlesfoam_amd.api import Context
    from cudaparticlesfoam_amd.cases import pitzdaily as pz
    from cudaparticlesfoam_amd.parallel import x_slab_renumbering
    dev = torch.device("cuda", 0)
    n = a.particles
    mesh0 = pz.pitzdaily_mesh(); c0, _ = mesh0.cell_centres_volumes()
    mesh = mesh0.renumber_cells(x_slab_renumbering(c0))
    U = pz.uniform_u(mesh)
    sink = mesh.patch_cells("outlet")
    (lx, ly, lz), (hx, hy, hz) = pz.DOMAIN_BOX
    box = ((lx, ly, lz), (lx + 0.05 * (hx - lx), hy, hz))          # the inlet end; a draw below the step stays dead for an epoch
    cc, _ = mesh.cell_centres_volumes()
    along = (cc[:, 0] - lx) / (hx - lx)
    maps = {k: np.clip(np.floor(along * k), 0, k - 1).astype(np.int32) for k in (4, 63)}
    ctxs = {}
    xyz = None
    for name in ("slab4", "slab63", "dense", "off"):
        ctx = Context(0); ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.set_option("stats", 0); ctx.set_option("sort_interval", SORT_EVERY)
        ctx.set_mesh(mesh); ctx.set_velocity(U)
        if xyz is None:
            x, y, z, _ = bench.seed_in_fluid(ctx, torch, n, pz.DOMAIN_BOX, 1000, dev)
            xyz = torch.stack([x, y, z], 1).cpu().numpy()
            del x, y, z
        ctx.set_particles(xyz); ctx.locate_initial(); ctx.sort_by_cell()
        ctx.set_sink_cells(sink)
        if name in ("slab4", "off"):
            ctx.age_enable(SORT_EVERY, 64)
        if name == "dense":
            ctx.exposure_enable(DT * SORT_EVERY, 64); ctx.set_exposure_field(1.0 + along)
        if name in ("slab4", "slab63"):
            k = 4 if name == "slab4" else 63
            ctx.zone_enable(k); ctx.set_zone_map(maps[k])
        ctxs[name] = ctx
    slab4, slab63, dense, off = (ctxs[k] for k in ("slab4", "slab63", "dense", "off"))
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
        timed("step", group if since else None, lambda: slab4.step(DT, D, 1))
        for c in (slab63, dense, off):
            c.step(DT, D, 1)
        timed("sample_4", group, slab4.zone_sample)
        timed("sample_63", group, slab63.zone_sample)
        timed("accumulate_dense", group, lambda: dense.exposure_accumulate(DT))
        timed("sink_zoned", group, slab4.sink_apply)
        timed("sink_twin", group, off.sink_apply)
        slab63.sink_apply(); dense.sink_apply()
        timed("respawn_stamp", group, lambda: slab4.respawn_box(box[0], box[1], -1))
        timed("respawn_twin", group, lambda: off.respawn_box(box[0], box[1], -1))
        slab63.respawn_box(box[0], box[1], -1); dense.respawn_box(box[0], box[1], -1)
        timed("occupancy", group, slab4.occupancy_sample)
        timed("age_sample", group, slab4.age_sample)

    for k in range(STEADY_CYCLES):
        cycle(k, False)
    torch.cuda.synchronize()
    steady = slab4.recycle_counts()
    f0 = slab4.zone_flows()[0].astype(np.int64)
    for k in range(STEADY_CYCLES, STEADY_CYCLES + a.periods * SORT_EVERY):
        cycle(k, True)
    torch.cuda.synchronize()
    out = dict(case="pitz", particles=n, cells=mesh.n_cells, sink_cells=int(sink.size), D=D, dt=DT, periods=a.periods,
               sort_every=SORT_EVERY, steady_cycles=STEADY_CYCLES, absorbed_per_cycle=steady["absorbed"] / STEADY_CYCLES,
               last_table_bytes=n, step_kernel=slab4.step_kernel_name(D, 0))
    for group in ("fresh", "stale"):
        g = {}
        for (name, grp), pairs in rows.items():
            if grp == group:
                ms = sorted(e0.elapsed_time(e1) for e0, e1 in pairs)
                g[name] = dict(ms=round(ms[len(ms) // 2], 5), min_ms=round(ms[0], 5), max_ms=round(ms[-1], 5), samples=len(ms))
        for kind in ("sample_4", "sample_63"):
            for other in ("age_sample", "accumulate_dense", "occupancy", "step"):
                g["%s_over_%s" % (kind, other)] = round(g[kind]["ms"] / g[other]["ms"], 3)
        g["sink_zoned_over_twin"] = round(g["sink_zoned"]["ms"] / g["sink_twin"]["ms"], 3)
        g["sink_zoned_minus_twin_ms"] = round(g["sink_zoned"]["ms"] - g["sink_twin"]["ms"], 5)
        g["respawn_stamp_minus_twin_ms"] = round(g["respawn_stamp"]["ms"] - g["respawn_twin"]["ms"], 5)
        out[group] = g
    # the four runs are one run: zones changed nothing of the cloud
    ref = off.get_particles()
    same = True
    for c in (slab4, slab63, dense):
        p = c.get_particles()
        same = same and bool(np.array_equal(p[0].view(np.int64), ref[0].view(np.int64)) and np.array_equal(p[1], ref[1])
                             and c.recycle_counts() == off.recycle_counts())
    out["runs_identical"] = same
    out["age_histograms_identical"] = bool(np.array_equal(slab4.age_histogram(), off.age_histogram()))
    # what the timed part counted: the share of samples that changed a particle's zone (a store), and the books
    f4 = slab4.zone_flows()[0].astype(np.int64) - f0
    out["samples_counted"] = int(f4[:, :4].sum())
    out["share_of_samples_that_store_4"] = round(float(f4[:, :4].sum() - np.trace(f4[:4, :4])) / float(max(f4[:, :4].sum(), 1)), 5)
    f63, ns = slab63.zone_flows()
    f63 = f63.astype(np.int64)
    out["share_of_samples_that_store_63"] = round(float(f63[:, :63].sum() - np.trace(f63[:63, :63])) / float(max(f63[:, :63].sum(), 1)), 5)
    out["n_samples"] = int(ns)
    out["left_equals_absorbed"] = bool(int(f63[:, 63].sum()) == slab63.recycle_counts()["absorbed"])
    out["residence_s_4"] = [None if not np.isfinite(v) else round(float(v), 6) for v in slab4.zone_residence(DT)]
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    for c in ctxs.values():
        c.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--worker", action="store_true", help="(internal) run the workload in this process")
    ap.add_argument("--particles", type=int, default=10_000_000)
    ap.add_argument("--periods", type=int, default=8, help="sort periods of 25 cycles that are timed")
    ap.add_argument("--seconds", type=int, default=400, help="time limit of the workload's process")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.periods < 4:
        ap.error("--periods: at least 4")
    if a.worker:
        return worker(a)
    cmd = ["timeout", "-k", "10", str(a.seconds), sys.executable, os.path.abspath(__file__), "--worker", "--particles", str(a.particles),
           "--periods", str(a.periods)] + (["--out", a.out] if a.out else [])
    sys.exit(subprocess.run(cmd).returncode)


if __name__ == "__main__":
    main()
