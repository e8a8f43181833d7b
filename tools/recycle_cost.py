#!/usr/bin/env python3
"""Developer tool (GPU box): what recycling (cpf_sink_apply*, cpf_respawn_box*; csrc/cpf_recycle.hip) costs next to an occupancy
sample -- the same 4-byte-per-particle read -- and next to a step.  The pitzDaily 1e7-particle cloud as bench.py builds it, D =
1.5e-5, sink = the outlet patch's owner cells, source = the inlet end of the domain box; in a process of its own under its own time
limit.  First the cloud is brought to steady recycling (cycles of step, sink, respawn of all, re-sorted every 25), then, fresh from
a sort and again 25 cycles of diffusion past it:
  (a) cpf_occupancy_sample_dev, (b) cpf_sink_apply_dev with nothing left to absorb -- both as 50 back-to-back launches between two
      events, three repeats alternating, the median --,
  (c) cpf_sink_apply_dev with its absorptions, (d) cpf_respawn_box_dev of all dead slots with 1 % of the cloud dead (scattered over
      the array, and at its tail, where a sort leaves them), (e) the same limited to half of them -- the cell array is restored
      from a copy before every launch, and the figure is 50 x (restore, launch) back to back minus 50 x restore back to back,
      the median of three such differences --,
  (f) the step launch.
  python tools/recycle_cost.py [--out FILE.jsonl] [--launches 50] [--seconds 400]        prints one JSON line"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
D, DT, STALE_CYCLES, STEADY_CYCLES, SORT_EVERY = 1.5e-5, 1e-4, 25, 200, 25


def worker(a):
    import torch
    from _cases import make_case
    from _spinup import device_spinup
    from cudaparticlesfoam_amd.api import Context
    from cudaparticlesfoam_amd.cases import pitzdaily as pz
    dev = torch.device("cuda", 0)
    ctx = Context(0); ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    n = a.particles
    mesh, x, y, z, c, _ = make_case("pitz", ctx, torch, n, dev)
    p = lambda t: t.data_ptr()   # noqa: E731
    ctx.set_option("stats", 0)
    g = torch.arange(n, dtype=torch.int64, device=dev)
    sink = mesh.patch_cells("outlet")
    ctx.set_sink_cells(sink)
    (lx, ly, lz), (hx, hy, hz) = pz.DOMAIN_BOX
    box = ((lx, ly, lz), (lx + 0.05 * (hx - lx), hy, hz))          # the inlet end; a draw below the step stays dead for an epoch
    ctx.sort_by_cell_dev(p(x), p(y), p(z), p(c), p(g), n)
    device_spinup(ctx, torch, x, y, z, c, n, DT)
    # steady recycling
    for k in range(STEADY_CYCLES):
        ctx.step_dev(p(x), p(y), p(z), p(c), p(g), None, n, DT, D, k, 1, 0)
        ctx.sink_apply_dev(p(c), n)
        ctx.respawn_box_dev(p(x), p(y), p(z), p(c), p(g), n, box[0], box[1], -1, k)
        if (k + 1) % SORT_EVERY == 0:
            ctx.sort_by_cell_dev(p(x), p(y), p(z), p(c), p(g), n)
    torch.cuda.synchronize()
    steady = ctx.recycle_counts()
    ctx.recycle_reset_counts()

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

    def timed_each(restore, f):
        """ms per launch of f with `restore` before each: (restore, f) back to back minus restore alone back to back, the
        median of three such differences -- no host wait between the launches, so the device stays at its clocks"""
        def both():
            restore(); f()
        d = sorted(timed(both) - timed(restore) for _ in range(3))
        return round(d[1], 5)

    def measure(x0, y0, z0, c0):
        """on scratch copies of the cloud (x0, y0, z0, c0)"""
        sx, sy, sz, sc = x0.clone(), y0.clone(), z0.clone(), c0.clone()
        out = {}
        live = sc.clone()
        ctx.sink_apply_dev(p(live), n)                              # (what a pass finds when the sink has just been applied)
        rows = {"occupancy_sample_dev": [], "sink_apply_nothing_to_absorb": []}
        for _ in range(3):
            rows["occupancy_sample_dev"].append(timed(lambda: ctx.occupancy_sample_dev(p(live), n)))
            rows["sink_apply_nothing_to_absorb"].append(timed(lambda: ctx.sink_apply_dev(p(live), n)))
        out.update({k: dict(ms=round(sorted(v)[1], 5), repeats_ms=[round(t, 5) for t in v]) for k, v in rows.items()})
        out["sink_over_occupancy"] = round(out["sink_apply_nothing_to_absorb"]["ms"] / out["occupancy_sample_dev"]["ms"], 3)
        before = ctx.recycle_counts()["absorbed"]
        out["sink_apply_absorbing_ms"] = timed_each(lambda: sc.copy_(c0), lambda: ctx.sink_apply_dev(p(sc), n))
        out["absorbed_per_apply"] = (ctx.recycle_counts()["absorbed"] - before) // (3 * (a.launches + 5))
        n_dead = n // 100
        for where in ("scattered", "tail"):
            dead = live.clone()
            if where == "scattered":
                dead[torch.randperm(n, device=dev)[:n_dead]] = -1
            else:
                dead[n - n_dead:] = -1
            epoch = [0]

            def respawn(limit):
                ctx.respawn_box_dev(p(sx), p(sy), p(sz), p(sc), p(g), n, box[0], box[1], limit, epoch[0]); epoch[0] += 1
            out["respawn_all_1pct_%s_ms" % where] = timed_each(lambda: sc.copy_(dead), lambda: respawn(-1))
            out["respawn_limited_half_1pct_%s_ms" % where] = timed_each(lambda: sc.copy_(dead), lambda: respawn(n_dead // 2))
        # the cloud's own dead: the draws of the last respawn that fell outside the mesh, in a run where the sink's cells are
        out["dead_in_cloud"] = int((live < 0).sum())
        out["respawn_all_own_dead_ms"] = timed_each(lambda: sc.copy_(live), lambda: ctx.respawn_box_dev(
            p(sx), p(sy), p(sz), p(sc), p(g), n, box[0], box[1], -1, 0))
        none = torch.clamp(live, min=0)
        out["respawn_nothing_dead_ms"] = timed_each(lambda: sc.copy_(none), lambda: ctx.respawn_box_dev(
            p(sx), p(sy), p(sz), p(sc), p(g), n, box[0], box[1], -1, 0))
        return out

    out = dict(case="pitz", particles=n, cells=mesh.n_cells, sink_cells=int(sink.size), launches=a.launches, D=D, dt=DT,
               id_bytes=4 * n, id_bound_ms_at_6_TBps=round(4 * n / 6.0e12 * 1e3, 5), steady_cycles=STEADY_CYCLES,
               steady_counts=steady, absorbed_per_cycle=steady["absorbed"] / STEADY_CYCLES)
    out["sorted"] = measure(x, y, z, c)
    sx, sy, sz, sc = x.clone(), y.clone(), z.clone(), c.clone()
    step = [0]

    def one_step():
        ctx.step_dev(p(sx), p(sy), p(sz), p(sc), p(g), None, n, DT, D, step[0], 1, 0); step[0] += 1
    out["step_launch_ms"] = round(timed(one_step), 5)
    out["step_kernel"] = ctx.step_kernel_name(D, 0)
    sx, sy, sz, sc = x.clone(), y.clone(), z.clone(), c.clone()
    ctx.step_dev(p(sx), p(sy), p(sz), p(sc), p(g), None, n, DT, D, 0, STALE_CYCLES, 0)
    out["stale_%d_cycles" % STALE_CYCLES] = measure(sx, sy, sz, sc)
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
