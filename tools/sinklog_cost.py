#!/usr/bin/env python3
"""Developer tool (GPU box): what the sink log (cpf_sink_log_*; csrc/cpf_sinklog.hip) adds to cpf_sink_apply, and what a read of
one apply's records costs.  The pitzDaily 1e7-particle cloud as bench.py seeds it, D = 1.5e-5, sink = the outlet patch's owner
cells, source = the inlet end of the domain box: tools/zones_cost.py's regime and its method -- FOUR contexts run the same recycled
run in lockstep on one stream (the runs are bit-identical: the tool checks it), so at every cycle all hold the same arrays, and
each call is bracketed by a pair of events:
  off      no log, no group: the twin of `log`
  log      the log alone
  groups   age, tags, routes, exposure and zones, no log: the twin of `full`
  full     the log and all five groups
  cycle = step (1 cycle), accumulate and zone sample (groups, full), sink, respawn of all dead; every cloud re-sorts every 25
  cycles.  The logs are cleared behind every apply (outside the brackets).
First 200 cycles to steady recycling, then --periods sort periods are timed.  Per call the median, minimum and maximum over the
timed cycles that are "fresh" (the first 3 after a sort) and over those that are "stale" (the last 3 before the next):
  sink_off / sink_log / sink_groups / sink_full     cpf_sink_apply of the four
Then --reads more cycles, in each of which `log`'s and `full`'s records of that one apply are read (cpf_sink_log_read: the
synchronisation, the copy and the sort on the host), timed on the host's clock behind a synchronisation of its own.
An event pair round one launch carries the launch gap with it: the figures are call times on a busy stream, not kernel times.
  python tools/sinklog_cost.py [--out FILE.jsonl] [--periods 8] [--seconds 500]        prints one JSON line"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
D, DT, STEADY_CYCLES, SORT_EVERY, EDGE = 1.5e-5, 1e-4, 200, 25, 3
NAMES = ("off", "log", "groups", "full")


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
    zone_map = np.clip(np.floor(along * 4), 0, 3).astype(np.int32)
    capacity = max(n // 20, 1024)                                   # an apply absorbs a third of a per cent of the cloud
    ctxs = {}
    xyz = None
    for name in NAMES:
        ctx = Context(0); ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ctx.set_option("stats", 0); ctx.set_option("sort_interval", SORT_EVERY)
        ctx.set_mesh(mesh); ctx.set_velocity(U)
        if xyz is None:
            x, y, z, _ = bench.seed_in_fluid(ctx, torch, n, pz.DOMAIN_BOX, 1000, dev)
            xyz = torch.stack([x, y, z], 1).cpu().numpy()
            del x, y, z
        ctx.set_particles(xyz); ctx.locate_initial(); ctx.sort_by_cell()
        ctx.set_sink_cells(sink)
        if name in ("groups", "full"):
            ctx.age_enable(SORT_EVERY, 64)
            ctx.tag_enable(2, 2); ctx.set_sink_groups(sink, np.arange(sink.size) % 2); ctx.set_box_origin(1)
            ctx.route_enable()
            ctx.exposure_enable(DT * SORT_EVERY, 64); ctx.set_exposure_field(1.0 + along)
            ctx.zone_enable(4); ctx.set_zone_map(zone_map)
        if name in ("log", "full"):
            ctx.sink_log_enable(capacity)
        ctxs[name] = ctx
    off, log, groups, full = (ctxs[k] for k in NAMES)
    rows = {}
    dropped = 0

    def timed(name, group, f):
        if group is None:
            return f()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); f(); e1.record()
        rows.setdefault((name, group), []).append((e0, e1))

    def cycle(k, timing, clear=True):
        since = (k + 1) % SORT_EVERY                                # cycles since a sort, behind this cycle's step (0: it ended in one)
        group = None if not timing else "fresh" if since < EDGE else "stale" if since >= SORT_EVERY - EDGE else None
        for c in ctxs.values():
            c.step(DT, D, 1)
        for c in (groups, full):
            c.exposure_accumulate(DT); c.zone_sample()
        timed("sink_off", group, off.sink_apply)
        timed("sink_log", group, log.sink_apply)
        timed("sink_groups", group, groups.sink_apply)
        timed("sink_full", group, full.sink_apply)
        for c in ctxs.values():
            c.respawn_box(box[0], box[1], -1)
        if clear:
            log.sink_log_clear(); full.sink_log_clear()

    for k in range(STEADY_CYCLES):
        cycle(k, False)
    torch.cuda.synchronize()
    steady = off.recycle_counts()
    last = STEADY_CYCLES + a.periods * SORT_EVERY
    for k in range(STEADY_CYCLES, last):
        cycle(k, True)
    torch.cuda.synchronize()
    out = dict(case="pitz", particles=n, cells=mesh.n_cells, sink_cells=int(sink.size), D=D, dt=DT, periods=a.periods,
               sort_every=SORT_EVERY, steady_cycles=STEADY_CYCLES, absorbed_per_cycle=steady["absorbed"] / STEADY_CYCLES,
               record_bytes=64, capacity=capacity, step_kernel=off.step_kernel_name(D, 0))
    for group in ("fresh", "stale"):
        g = {}
        for (name, grp), pairs in rows.items():
            if grp == group:
                ms = sorted(e0.elapsed_time(e1) for e0, e1 in pairs)
                g[name] = dict(ms=round(ms[len(ms) // 2], 5), min_ms=round(ms[0], 5), max_ms=round(ms[-1], 5), samples=len(ms))
        g["sink_log_minus_off_ms"] = round(g["sink_log"]["ms"] - g["sink_off"]["ms"], 5)
        g["sink_full_minus_groups_ms"] = round(g["sink_full"]["ms"] - g["sink_groups"]["ms"], 5)
        out[group] = g
    # the reads: one apply's records each, on the host's clock
    reads = {"log": [], "full": []}
    records = []
    for k in range(last, last + a.reads):
        cycle(k, False, clear=False)
        torch.cuda.synchronize()
        for name, c in (("log", log), ("full", full)):
            t0 = time.perf_counter()
            rec = c.sink_log_read()
            reads[name].append((time.perf_counter() - t0) * 1e3)
            dropped += c.sink_log_counts()[1]
            c.sink_log_clear()
        records.append(int(rec.size))
    for name, ms in reads.items():
        ms = sorted(ms)
        out["read_" + name] = dict(ms=round(ms[len(ms) // 2], 4), min_ms=round(ms[0], 4), max_ms=round(ms[-1], 4), samples=len(ms))
    out["records_per_read"] = sorted(records)[len(records) // 2]
    out["dropped"] = int(dropped)
    # the four runs are one run: the log changed nothing of the cloud, nor of the groups' tables
    ref = off.get_particles()
    same = True
    for c in (log, groups, full):
        p = c.get_particles()
        same = same and bool(np.array_equal(p[0].view(np.int64), ref[0].view(np.int64)) and np.array_equal(p[1], ref[1])
                             and c.recycle_counts() == off.recycle_counts())
    out["runs_identical"] = same
    out["tables_identical"] = bool(np.array_equal(full.route_histogram(), groups.route_histogram())
                                   and np.array_equal(full.dose_histogram(), groups.dose_histogram())
                                   and np.array_equal(full.zone_flows()[0], groups.zone_flows()[0])
                                   and np.array_equal(full.age_histogram(), groups.age_histogram())
                                   and np.array_equal(full.transfer(), groups.transfer()))
    # the last read's records against the tables' own rules: a median no histogram gives
    out["median_age_cycles_last_read"] = float(np.median(rec["age"])) if rec.size else None
    out["fields_last_read"] = sorted(int(v) for v in np.unique(rec["fields"]))
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
    ap.add_argument("--reads", type=int, default=10, help="cycles behind the timed ones in which one apply's records are read")
    ap.add_argument("--seconds", type=int, default=500, help="time limit of the workload's process")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.periods < 4:
        ap.error("--periods: at least 4")
    if a.reads < 1:
        ap.error("--reads: at least 1")
    if a.worker:
        return worker(a)
    cmd = ["timeout", "-k", "10", str(a.seconds), sys.executable, os.path.abspath(__file__), "--worker", "--particles", str(a.particles),
           "--periods", str(a.periods), "--reads", str(a.reads)] + (["--out", a.out] if a.out else [])
    sys.exit(subprocess.run(cmd).returncode)


if __name__ == "__main__":
    main()
