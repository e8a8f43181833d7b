#!/usr/bin/env python3
"""Developer tool (GPU box): what exposure (cpf_exposure_*; csrc/cpf_exposure.hip) costs next to the kernels it rides on.  The
pitzDaily 1e7-particle cloud as bench.py seeds it, D = 1.5e-5, sink = the outlet patch's owner cells, source = the inlet end of the
domain box: tools/age_cost.py's regime and its method -- FOUR contexts run the same recycled run in lockstep on one stream (the runs
are bit-identical: the tool checks it), so at every cycle all hold the same arrays, and each call is bracketed by a pair of events:
  dense   exposure with a positive rate in every cell, and age tracking (for the age sample next to it)
  zone    exposure with rate 1 in the outlet's cells and 0 elsewhere: the time spent in a marked zone
  zero    exposure with the field it has at enable, all zero
  off     no exposure, age tracking: the twin of `dense`
  cycle = step (1 cycle), accumulate, sink, respawn of all dead, occupancy sample, age sample; every cloud re-sorts every 25 cycles.
First 200 cycles to steady recycling, then --periods sort periods are timed.  Per call the median, minimum and maximum over the
timed cycles that are "fresh" (the first 3 after a sort) and over those that are "stale" (the last 3 before the next):
  accumulate_dense / _zone / _zero   cpf_exposure_accumulate of the three
  age_sample / occupancy / step      cpf_age_sample, cpf_occupancy_sample and the step launch of `dense`: the neighbours
  sink_exposed / sink_twin           cpf_sink_apply of `dense` (the dose pass, then the age pass) and of `off` (the age pass)
  respawn_stamp / respawn_twin       cpf_respawn_box of `dense` (age's stamp, the dose stamp, the respawn) and of `off`
An event pair round one launch carries the launch gap with it: the figures are call times on a busy stream, not kernel times.
  python tools/exposure_cost.py [--out FILE.jsonl] [--periods 8] [--seconds 400]        prints one JSON line"""
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
    fields = dict(dense=1.0 + (cc[:, 0] - lx) / (hx - lx), zone=np.zeros(mesh.n_cells), zero=None)
    fields["zone"][sink] = 1.0
    ctxs = {}
    xyz = None
    for name in ("dense", "zone", "zero", "off"):
        ctx = Context(0); ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.set_option("stats", 0); ctx.set_option("sort_interval", SORT_EVERY)
        ctx.set_mesh(mesh); ctx.set_velocity(U)
        if xyz is None:
            x, y, z, _ = bench.seed_in_fluid(ctx, torch, n, pz.DOMAIN_BOX, 1000, dev)
            xyz = torch.stack([x, y, z], 1).cpu().numpy()
            del x, y, z
        ctx.set_particles(xyz); ctx.locate_initial(); ctx.sort_by_cell()
        ctx.set_sink_cells(sink)
        if name in ("dense", "off"):
            ctx.age_enable(SORT_EVERY, 64)
        if name != "off":
            ctx.exposure_enable(DT * SORT_EVERY, 64)
            if fields[name] is not None:
                ctx.set_exposure_field(fields[name])
        ctxs[name] = ctx
    dense, zone, zero, off = (ctxs[k] for k in ("dense", "zone", "zero", "off"))
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
        timed("step", group if since else None, lambda: dense.step(DT, D, 1))
        for c in (zone, zero, off):
            c.step(DT, D, 1)
        timed("accumulate_dense", group, lambda: dense.exposure_accumulate(DT))
        timed("accumulate_zone", group, lambda: zone.exposure_accumulate(DT))
        timed("accumulate_zero", group, lambda: zero.exposure_accumulate(DT))
        timed("sink_exposed", group, dense.sink_apply)
        timed("sink_twin", group, off.sink_apply)
        zone.sink_apply(); zero.sink_apply()
        timed("respawn_stamp", group, lambda: dense.respawn_box(box[0], box[1], -1))
        timed("respawn_twin", group, lambda: off.respawn_box(box[0], box[1], -1))
        zone.respawn_box(box[0], box[1], -1); zero.respawn_box(box[0], box[1], -1)
        timed("occupancy", group, dense.occupancy_sample)
        timed("age_sample", group, dense.age_sample)

    for k in range(STEADY_CYCLES):
        cycle(k, False)
    torch.cuda.synchronize()
    steady = dense.recycle_counts()
    for k in range(STEADY_CYCLES, STEADY_CYCLES + a.periods * SORT_EVERY):
        cycle(k, True)
    torch.cuda.synchronize()
    out = dict(case="pitz", particles=n, cells=mesh.n_cells, sink_cells=int(sink.size), D=D, dt=DT, periods=a.periods,
               sort_every=SORT_EVERY, steady_cycles=STEADY_CYCLES, absorbed_per_cycle=steady["absorbed"] / STEADY_CYCLES,
               dose_table_bytes=8 * n, step_kernel=dense.step_kernel_name(D, 0))
    for group in ("fresh", "stale"):
        g = {}
        for (name, grp), pairs in rows.items():
            if grp == group:
                ms = sorted(e0.elapsed_time(e1) for e0, e1 in pairs)
                g[name] = dict(ms=round(ms[len(ms) // 2], 5), min_ms=round(ms[0], 5), max_ms=round(ms[-1], 5), samples=len(ms))
        for kind in ("dense", "zone", "zero"):
            for other in ("age_sample", "occupancy", "step"):
                g["accumulate_%s_over_%s" % (kind, other)] = round(g["accumulate_" + kind]["ms"] / g[other]["ms"], 3)
        g["sink_exposed_over_twin"] = round(g["sink_exposed"]["ms"] / g["sink_twin"]["ms"], 3)
        g["sink_exposed_minus_twin_ms"] = round(g["sink_exposed"]["ms"] - g["sink_twin"]["ms"], 5)
        g["respawn_stamp_minus_twin_ms"] = round(g["respawn_stamp"]["ms"] - g["respawn_twin"]["ms"], 5)
        out[group] = g
    # the four runs are one run: exposure changed nothing of the cloud
    ref = off.get_particles()
    same = True
    for c in (dense, zone, zero):
        p = c.get_particles()
        same = same and bool(np.array_equal(p[0].view(np.int64), ref[0].view(np.int64)) and np.array_equal(p[1], ref[1])
                             and c.recycle_counts() == off.recycle_counts())
    out["runs_identical"] = same
    out["age_histograms_identical"] = bool(np.array_equal(dense.age_histogram(), off.age_histogram()))
    hist = dense.dose_histogram()
    out["dose_absorbed"] = int(hist.sum()); out["dose_bins_used"] = int((hist > 0).sum())
    out["absorbed"] = int(dense.recycle_counts()["absorbed"])
    # the zone is the sink: who gets a dose there is absorbed in the same cycle, with one cycle's worth, and leaves it in bin 0
    hz = zone.dose_histogram()
    out["zone_dose_absorbed"] = int(hz.sum()); out["zone_dose_bins_used"] = int((hz > 0).sum())
    out["zero_doses_all_zero"] = bool(not (zero.doses() > 0).any())
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
