"""GPU: cpf_set_option, key by key (include/cpf.h), and the lifetime of the "VertexVelocity" tables.

Every one of the 23 keys takes a value of its range; the 21 that check their value refuse one outside it (and a fraction, where
the option is a whole number) with CPF_ERR_ARG and a message that names the key; "stream_debug" and "stats" take anything.  The
ranges are written out here, from include/cpf.h, not read from the library.  Where the library has an accessor, an accepted
option shows: cpf_step_kernel_name for what decides the step kernel, cpf_get_mesh_flags, cpf_get_mesh_quality, the timing
counters, the frame file."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# key: (accepted, refused).  The first accepted value is set once more at the end: the default, where the range holds it.
RANGES = {
    "step_variant": ([-1, 0, 3, 4], [-2, 6, 0.5, float("nan")]),
    "vertex_fast": ([1, 0], [-1, 2, 0.5]),
    "z_fold": ([1, 0], [-1, 2, 0.5]),
    "mixed_records": ([1, 0], [-1, 2, 0.5]),
    "flat_walk": ([1, 0], [-1, 2, 0.5]),
    "flat_z": ([1, 0], [-1, 2, 0.5]),
    "box_records": ([1, 0], [-1, 2, 0.5]),
    "stream_tiles_per_chunk": ([3, 1, 1024], [0, 1025, 2.5, -1]),
    "stream_tail_fraction": ([0.1, 0.0, 1.0, 0.25], [-0.01, 1.01, float("nan")]),
    "coop_max_cells": ([0, 1000, 1 << 24], [-1, (1 << 24) + 1]),
    "stream_lookup": ([-1, 0, 1, 2, 3, 4, 5, 6], [-2, 7, 8, 0.5, -0.5]),
    "stream_lookup_by_density": ([0, 1], [-1, 2, 0.5]),
    "sort_method": ([2, 0], [1, 3, -1, 0.5]),
    "sort_curve": ([-1, 0, 1], [-2, 2, 0.5]),
    "vtu_binary": ([0, 1], [-1, 2, 0.5]),
    "stream_waves_per_cu": ([0, 1, 32], [-1, 33, 1.5]),
    "sort_interval": ([50, 0, 1e9], [-1, 2e9]),
    "timing_stride": ([1, 7, 1e6], [0, 1e6 + 1, 1.5]),
    "nonplanar_tol": ([1e-11, 1e-300, 1.0], [0.0, -1e-11, float("inf"), float("nan")]),
    "split_nonplanar": ([1, 0], [-1, 2, 0.5]),
}
UNCHECKED = {"stream_debug": [0, 1, 2, -7, 0.5], "stats": [1, 0, 3, -1, 0.5]}
SORT_KEY_BITS = ([222, 0, 444, 912, 30], [-1, 445, 1000, 2.5])        # (needs a mesh: below)


def _refused(ctx, key, value, status, word):
    from cudaparticlesfoam_amd import _lib as L
    with pytest.raises(L.CpfError) as e:
        ctx.set_option(key, value)
    assert e.value.status == status and word in str(e.value), (key, value, str(e.value))


def test_all_23_keys_ranges_and_messages(gpu_ctx_factory, pitz):
    from cudaparticlesfoam_amd import _lib as L
    assert len(RANGES) + len(UNCHECKED) + 1 == 23
    ctx = gpu_ctx_factory()
    for key, (good, bad) in RANGES.items():
        for v in bad:
            _refused(ctx, key, v, L.CPF_ERR_ARG, key)
        for v in good + good[:1]:
            ctx.set_option(key, v)
    for v in (1, 2, 5):                     # experiments: refused by name in the default build, accepted with EXPERIMENTS=1
        try:
            ctx.set_option("step_variant", v)
        except L.CpfError as e:
            assert e.status == L.CPF_ERR_ARG and "step_variant" in str(e) and "EXPERIMENTS=1" in str(e)
    ctx.set_option("step_variant", -1)
    for key, values in UNCHECKED.items():
        for v in values + values[:1]:
            ctx.set_option(key, v)
    # "sort_key_bits" rescales the mesh's sort boxes: no mesh, no option -- whatever the value
    for v in SORT_KEY_BITS[0] + SORT_KEY_BITS[1]:
        _refused(ctx, "sort_key_bits", v, L.CPF_ERR_STATE, "sort_key_bits: call cpf_set_mesh first")
    ctx.set_mesh(pitz["mesh"])
    for v in SORT_KEY_BITS[1]:
        _refused(ctx, "sort_key_bits", v, L.CPF_ERR_ARG, "sort_key_bits")
    for v in SORT_KEY_BITS[0]:
        ctx.set_option("sort_key_bits", v)
    for key in ("nope", "", "stats ", "Stats", "sort_key_bit"):
        with pytest.raises(L.CpfError) as e:
            ctx.set_option(key, 1)
        assert e.value.status == L.CPF_ERR_ARG and str(e.value).endswith("cpf_set_option: unknown key '%s'" % key)


def test_accepted_options_show(gpu_ctx_factory, pitz, tmp_path):
    from cudaparticlesfoam_amd import _lib as L
    pz, mesh = pitz["pz"], pitz["mesh"]
    ctx = gpu_ctx_factory()
    ctx.set_option("nonplanar_tol", 3e-9)                       # read at cpf_set_mesh
    ctx.set_mesh(mesh); ctx.set_velocity(pitz["U_uniform"])
    assert ctx.mesh_quality()["tol"] == 3e-9
    xyz = pz.uniform_points(7, 200_000, *pz.DOMAIN_BOX)         # 16 particles per cell: neither sparse nor the loop lookup
    ctx.set_particles(xyz); ctx.locate_initial()
    name = lambda flags=0: ctx.step_kernel_name(0.0, flags)     # noqa: E731
    # "stats": the kernel's STATS argument (the fixture switched it on)
    assert name() == "cpf::step_kernel_stream<false, true, false, true, 9>"
    ctx.set_option("stats", 0)
    assert name() == "cpf::step_kernel_stream<false, true, false, false, 9>"
    # "flat_walk", "stream_lookup": the LOOKUP argument
    ctx.set_option("flat_walk", 0)
    assert name().endswith(", 1>")
    for v, want in ((0, 0), (1, 1), (4, 4), (6, 1), (-1, 1)):   # (6, box records: not on this mesh -- the fixed compare)
        ctx.set_option("stream_lookup", v)
        assert name() == "cpf::step_kernel_stream<false, true, false, false, %d>" % want
    ctx.set_option("flat_walk", 1)
    # "flat_z": behind a flat launch the cloud is settled, and the next launch is the body without z -- unless z is always streamed
    ctx.step(1e-4, 0.0, 1)
    assert name() == "cpf::step_kernel_stream_flat<true, false, false, 9>"
    ctx.set_option("flat_z", 0)
    assert name() == "cpf::step_kernel_stream<false, true, false, false, 9>"
    ctx.set_option("flat_z", 1)
    # "step_variant"
    for v, want in ((0, "cpf::step_kernel<0, false, true, false>"), (3, "cpf::step_kernel_coop<false, true, false, false>"),
                    (4, "cpf::step_kernel_stream_flat<true, false, false, 9>")):
        ctx.set_option("step_variant", v)
        assert name() == want
    ctx.set_option("step_variant", -1)
    # "z_fold": the mesh is one cell thick, and the walk uses it or not
    assert ctx.mesh_flags()["z_thin"] == 1
    ctx.set_option("z_fold", 0)
    assert ctx.mesh_flags()["z_thin"] == 0
    ctx.set_option("z_fold", 1)
    # "timing_stride": every k-th launch is bracketed
    ctx.set_option("timing_stride", 3)
    ctx.timing_enable(True)
    ctx.step(1e-4, 0.0, 7)
    assert ctx.timing_read()[0] == 3                            # launches 0, 3, 6
    ctx.timing_enable(False)
    ctx.set_option("timing_stride", 1)
    # "vtu_binary": the frame's arrays
    for binary in (0, 1):
        ctx.set_option("vtu_binary", binary)
        f = tmp_path / ("frame_%d.vtu" % binary)
        ctx.write_vtu(str(f))
        assert (b"Name='Position' format='ascii'" in f.read_bytes()) == (binary == 0)
    # "vertex_fast": the "VertexVelocity" cycle's locate
    centres, _ = mesh.cell_centres_volumes()
    pos, tets = mesh.tet_decomposition(centres)
    ctx.set_tets(pos, tets, 12); ctx.set_vertex_velocity(np.ones(pos.shape))
    assert "(cone locate)" in name(L.STEP_VERTEX_VELOCITY)
    ctx.set_option("vertex_fast", 0)
    assert "(all tets)" in name(L.STEP_VERTEX_VELOCITY)
    # "split_nonplanar" (read at cpf_set_mesh): a warped mesh is decomposed into tets or kept as given
    import warped as W
    from cudaparticlesfoam_amd.cases import box_mesh
    wm = W.warp_mesh(box_mesh(8, 7, 6, upper=(1.0, 1.0, 1.0)), 2e-2, seed=11)
    ctx.set_option("nonplanar_tol", 1e-11)
    for split in (1, 0):
        ctx.set_option("split_nonplanar", split)
        ctx.set_mesh(wm)
        q = ctx.mesh_quality()
        assert q["n_flagged"] > 0 and (q["n_derived"] > q["n_cells"]) == (split == 1)


def test_a_new_mesh_drops_the_tet_field(gpu_ctx_factory):
    """cpf_set_mesh -> cpf_set_tets -> cpf_set_vertex_velocity -> cpf_set_mesh: the decomposition belonged to the first mesh, a
    "VertexVelocity" step is refused until the second has its own -- and then gives the bits of a context that never saw the
    first."""
    from cudaparticlesfoam_amd import _lib as L
    from cudaparticlesfoam_amd.cases import box_mesh
    rng = np.random.default_rng(11)
    first = box_mesh(10, 9, 8)
    second = box_mesh(12, 7, 5, lower=(0.0, 0.0, 0.0), upper=(0.3, 0.05, 0.02), grading=(4.0, 0.3, 2.0))

    def tet_field(mesh):
        centres, _ = mesh.cell_centres_volumes()
        pos, tets = mesh.tet_decomposition(centres)
        return pos, tets

    pos2, tets2 = tet_field(second)
    vU2 = rng.normal(size=pos2.shape)
    lo, hi = second.bounds()
    P = rng.uniform(lo, hi, size=(50_000, 3))
    dt = 0.004 * float((hi - lo).min())

    def run(ctx):
        ctx.set_tets(pos2, tets2, 12); ctx.set_vertex_velocity(vU2)
        assert "(cone locate)" in ctx.step_kernel_name(0.0, L.STEP_VERTEX_VELOCITY)
        ctx.set_particles(P); ctx.locate_initial()
        ctx.step(dt, 0.0, 12, L.STEP_VERTEX_VELOCITY)
        return ctx.get_particles()

    used = gpu_ctx_factory()
    used.set_mesh(first); used.set_velocity(np.zeros((first.n_cells, 3)))
    pos1, tets1 = tet_field(first)
    used.set_tets(pos1, tets1, 12); used.set_vertex_velocity(rng.normal(size=pos1.shape))
    used.set_particles(rng.uniform(*first.bounds(), size=(1000, 3))); used.locate_initial()
    used.step(1e-3, 0.0, 2, L.STEP_VERTEX_VELOCITY)
    used.set_mesh(second); used.set_velocity(np.zeros((second.n_cells, 3)))
    used.set_particles(P); used.locate_initial()
    with pytest.raises(L.CpfError) as e:
        used.step(dt, 0.0, 1, L.STEP_VERTEX_VELOCITY)
    assert e.value.status == L.CPF_ERR_STATE and "cpf_set_tets" in str(e.value)
    with pytest.raises(L.CpfError) as e:                        # (velocities for the old decomposition have nowhere to go)
        used.set_vertex_velocity(np.ones(pos1.shape))
    assert e.value.status == L.CPF_ERR_STATE and "cpf_set_tets" in str(e.value)
    got = run(used)
    fresh = gpu_ctx_factory()
    fresh.set_mesh(second); fresh.set_velocity(np.zeros((second.n_cells, 3)))
    want = run(fresh)
    assert np.array_equal(got[0], want[0], equal_nan=True) and np.array_equal(got[1], want[1])
    assert np.abs(want[0][:, :3] - P).max() > 1e-4
