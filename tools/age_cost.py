#!/usr/bin/env python3
"""Developer tool (GPU box): what tracer age (cpf_age_*; csrc/cpf_age.hip) costs next to the kernels it rides on.  The pitzDaily
1e7-particle cloud as bench.py seeds it, D = 1.5e-5, sink = the outlet patch's owner cells, source = the inlet end of the domain box,
tools/recycle_cost.py's regime -- but on the CONTEXT-OWNED cloud, the only one the age entries know.  Its arrays cannot be restored
from a copy between launches, so the comparison is between TWO contexts that run the same recycled run in lockstep on one stream,
one with tracking and one without (the runs are bit-identical: the tool checks it): at every cycle both hold the same arrays, and
each call is bracketed by a pair of events.
  cycle = step (1 cycle), sink, respawn of all dead, occupancy sample[, age sample]; both clouds re-sort every 25 cycles.
First 200 cycles to steady recycling, then --periods sort periods are timed.  Per call the median over the timed cycles that are
"fresh" (the first 3 after a sort) and over those that are "stale" (the last 3 before the next):
  sink_plain / sink_ages        cpf_sink_apply without and with tracking, the same array
  respawn_plain / respawn_stamp cpf_respawn_box without and with the stamp pass before it
  occupancy / age_sample        cpf_occupancy_sample and cpf_age_sample of the tracked cloud
  step                          the step launch of the tracked cloud
An event pair round one launch carries the launch gap with it: the figures are call times on a busy stream, not kernel times.
  python tools/age_cost.py [--out FILE.jsonl] [--periods 8] [--seconds 400]        prints one JSON line"""
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
    ctxs = []
    xyz = None
    for track in (True, False):
        ctx = Context(0); ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.set_option("stats", 0); ctx.set_option("sort_interval", SORT_EVERY)
        ctx.set_mesh(mesh); ctx.set_velocity(U)
        if xyz is None:
            x, y, z, _ = bench.seed_in_fluid(ctx, torch, n, pz.DOMAIN_BOX, 1000, dev)
            xyz = torch.stack([x, y, z], 1).cpu().numpy()
            del x, y, z
        ctx.set_particles(xyz); ctx.locate_initial(); ctx.sort_by_cell()
        ctx.set_sink_cells(sink)
        if track:
            ctx.age_enable(SORT_EVERY, 64)
        ctxs.append(ctx)
    on, off = ctxs
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
        timed("step", group if since else None, lambda: on.step(DT, D, 1))
        off.step(DT, D, 1)
        timed("sink_ages", group, on.sink_apply)
        timed("sink_plain", group, off.sink_apply)
        timed("respawn_stamp", group, lambda: on.respawn_box(box[0], box[1], -1))
        timed("respawn_plain", group, lambda: off.respawn_box(box[0], box[1], -1))
        timed("occupancy", group, on.occupancy_sample)
        timed("age_sample", group, on.age_sample)
        off.occupancy_sample()

    for k in range(STEADY_CYCLES):
        cycle(k, False)
    torch.cuda.synchronize()
    steady = on.recycle_counts()
    on.age_reset()
    for k in range(STEADY_CYCLES, STEADY_CYCLES + a.periods * SORT_EVERY):
        cycle(k, True)
    torch.cuda.synchronize()
    out = dict(case="pitz", particles=n, cells=mesh.n_cells, sink_cells=int(sink.size), D=D, dt=DT, periods=a.periods,
               sort_every=SORT_EVERY, steady_cycles=STEADY_CYCLES, absorbed_per_cycle=steady["absorbed"] / STEADY_CYCLES,
               birth_table_bytes=4 * n, step_kernel=on.step_kernel_name(D, 0))
    for group in ("fresh", "stale"):
        g = {}
        for (name, grp), pairs in rows.items():
            if grp == group:
                ms = sorted(e0.elapsed_time(e1) for e0, e1 in pairs)
                g[name] = dict(ms=round(ms[len(ms) // 2], 5), min_ms=round(ms[0], 5), max_ms=round(ms[-1], 5), samples=len(ms))
        g["sink_ages_over_plain"] = round(g["sink_ages"]["ms"] / g["sink_plain"]["ms"], 3)
        g["respawn_stamp_minus_plain_ms"] = round(g["respawn_stamp"]["ms"] - g["respawn_plain"]["ms"], 5)
        g["age_sample_over_occupancy"] = round(g["age_sample"]["ms"] / g["occupancy"]["ms"], 3)
        g["age_sample_over_step"] = round(g["age_sample"]["ms"] / g["step"]["ms"], 3)
        out[group] = g
    # the two runs are one run: tracking changed nothing of the cloud
    a_, b_ = on.get_particles(), off.get_particles()
    out["runs_identical"] = bool(np.array_equal(a_[0].view(np.int64), b_[0].view(np.int64)) and np.array_equal(a_[1], b_[1])
                                 and on.recycle_counts() == off.recycle_counts())
    hist = on.age_histogram()
    s, c, ns = on.age_field()
    out["rtd_absorbed"] = int(hist.sum()); out["rtd_bins_used"] = int((hist > 0).sum())
    out["age_samples"] = int(ns)
    out["mean_age_cycles_max"] = float((s[c > 0] / c[c > 0]).max())
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")
    on.close(); off.close()


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
