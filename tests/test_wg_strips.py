"""The workgroup-row 2D kernel (kernels_2d_wg.hip) keeps six more positions of every input row in its ring (fetched by three
lanes of the last stage-0 wave), so that level 1 is complete on all 512 positions of a row and a strip yields 512 - 6 (K - 1)
output columns: 482 / 494 / 506 at 6 / 4 / 2 applications.  In strips on the grid's rim only the waves that hold a column
outside the interior run the EDGE copy of the step, beside waves of the same workgroup that run the interior copy, and the
halo values of a step are fetched right behind the barrier of the step before.  None of it may change a bit of the result.

Every case compares ONE launch of 6, 4 or 2 applications (lora_plan_stepn_region) BIT FOR BIT, over the whole padded buffer,
with single sweeps of a steps_per_launch = 1 plan driven as lora_plan_run's step-by-step loop drives them (buffer 0 carries
the caller's halo, buffer 1's halo is zero under the reference boundary or a copy of buffer 0's under the Dirichlet option).

Sizes (rows x columns):
  60 x 482    one strip at six applications whose last output column is the grid's last: lane 240's pair is the last one stored,
              and the six ring positions behind the row are the grid's right halo, clamped
  60 x 483    one column more: a second strip of a single column (six applications); at four and two applications one strip
  45 x 965    2 x 482 + 1: three strips at six applications, the middle one without a column outside the interior -- its
              windows of level 1 read the six extra ring positions as interior data of the next strip
  33 x 1500   four strips at six applications; 1500 = 3 x 494 + 18 = 2 x 506 + 488
In every rim strip wave 0 (left) or the wave that holds column n (right) runs EDGE and its neighbours do not.  Each size runs
with wg_rows small enough for three chunks per strip (checked through lora_debug_wg_layout) and with the launch's own rule.
Under the Dirichlet option a grid with an odd innermost extent has no fused launch (its plan runs the generic kernel): there
the case checks the refusal, and the even neighbours 60 x 484 and 45 x 966 run the Dirichlet launches.

Data: seeded integers 0..99 on star2d1r (nested-profile evaluation: the flagship's form; sums stay exact, so the structured
form and the direct taps of the single sweeps agree to the bit), and seeded normal doubles
  * on a full-rank 49-tap table, whose fused and single-sweep kernels apply the taps in the same order: against single sweeps;
  * on star2d1r against the row-streaming kernel (kernels_2d_stream.hip) in the same nested-profile form, four applications
    and / or two -- the taps reach every accumulator in the same order in both kernels, where the single sweeps' direct taps
    round differently.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [(60, 482), (60, 483), (45, 965), (33, 1500)]
THREE_CHUNKS = {60: 20, 45: 15, 33: 11}  # wg_rows: chunks of 22 / 15 / 15 rows at every depth
# (id, shape, full-rank table?, input, boundary, depths, reference)
CASES = [
    ("star2d1r_int", "star2d1r", False, "int", "reference", (6, 4, 2), "single"),
    ("taps49_normal", "box2d3r", True, "normal", "reference", (6, 4, 2), "single"),
    ("star2d1r_normal", "star2d1r", False, "normal", "reference", (6, 4, 2), "stream"),
    ("star2d1r_int_dirichlet", "star2d1r", False, "int", "dirichlet", (4, 2), "single"),
]
PARAMS = [(c, d) for c in CASES for d in SIZES + ([(60, 484), (45, 966)] if c[4] == "dirichlet" else [])]


@pytest.fixture(scope="module")
def L(engine_built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import lorastencil_amd as L

    assert L.device_count() >= 1
    return L


def taps49():
    """full rank, dyadic (as test_wg_own_pair.py): no structured form"""
    return np.random.default_rng(49).integers(-2, 3, 49).astype(np.float64) / 64.0


def bits(t):
    import torch

    return t.view(torch.int64)


def layout(plan, k, rows):
    from lorastencil_amd import _lib

    out = (ctypes.c_int * 8)()
    assert _lib.lib().lora_debug_wg_layout(plan._h, k, rows, 256, 2, out) == 0
    return list(out)


@pytest.mark.parametrize("case,dims", PARAMS, ids=[f"{c[0]}-{d[0]}x{d[1]}" for c, d in PARAMS])
def test_one_launch_is_the_single_sweeps_bit_for_bit(L, case, dims):
    import torch

    name, shape, full_rank, kind, bc, depths, reference = case
    m, n = dims
    if bc == "dirichlet" and n % 2:
        from lorastencil_amd import _lib

        plan = L.Plan(shape, dims).set_boundary(bc)
        assert plan.kernel_name == "stencil2d_generic_kernel" and plan.get_option("steps_per_launch") == 1
        a = torch.zeros(L.padded_shape(shape, dims), dtype=torch.float64, device="cuda")
        b = torch.zeros_like(a)
        for k in depths:
            with pytest.raises(L.LoraError) as e:
                plan.stepn_region(k, a, b, 0, m)
            assert e.value.status == _lib.LORA_EUNSUPPORTED, k
        return
    rng = np.random.default_rng(1000 * m + n + len(name))
    ps = L.padded_shape(shape, dims)
    host = rng.integers(0, 100, ps).astype(np.float64) if kind == "int" else rng.standard_normal(ps)
    u = torch.from_numpy(host).cuda()

    def make(options):
        plan = L.Plan(shape, dims)
        if full_rank:
            plan.set_weights(taps49())
        if bc == "dirichlet":
            plan.set_boundary(bc)
        for key, value in options.items():
            plan.set_option(key, value)
        return plan

    def launch(plan, k, src):
        got = u.clone()  # the halo a run leaves in every buffer; a launch writes the whole interior
        L.ops.interior(shape, got).fill_(float("nan"))
        plan.stepn_region(k, src, got, 0, m)
        torch.cuda.synchronize()
        return got

    want = {}
    if reference == "single":
        single = make({"steps_per_launch": 1})
        assert single.get_option("steps_per_launch") == 1 and "wg" not in single.kernel_name
        buf = [u.clone(), torch.zeros_like(u)]
        if bc == "dirichlet":
            single.halo(buf[1], "copy", buf[0])
        for k in range(1, max(depths) + 1):
            single.step(buf[(k - 1) % 2], buf[k % 2])
            if k in depths:
                want[k] = buf[k % 2].clone()  # (even k: buffer 0, whose halo is the caller's)
    else:
        s4, s2 = make({"steps_per_launch": 4}), make({"steps_per_launch": 2})
        for s in (s4, s2):
            assert s.kernel_name == "stencil2d_stream_kernel" and "eval=7," in s.kernel_signature, s.kernel_signature
        want[4] = launch(s4, 4, u)
        want[2] = launch(s2, 2, u)
        want[6] = launch(s2, 2, want[4])
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(w).all()) for w in want.values())

    for three_chunks in (True, False):
        plan = make({"wg_rows": THREE_CHUNKS[m]} if three_chunks else {})
        sig = plan.kernel_signature
        assert plan.kernel_name == "stencil2d_wg_kernel", sig
        assert plan.get_option("steps_per_launch") == max(depths), sig
        assert ("eval=7" in sig) == (shape == "star2d1r") and (not full_rank or "eval=2" in sig), sig
        for k in depths:
            strips, outw, rows_i, chunks_i, rows_e, chunks_e, wgs, rim = layout(plan, k, m)
            assert outw == 512 - 6 * (k - 1) and strips == -(-n // outw), (k, strips, outw)
            if three_chunks:
                assert chunks_e >= 3 and (strips == rim or chunks_i == 3), (k, chunks_i, chunks_e)
            got = launch(plan, k, u)
            differ = bits(got) != bits(want[k])
            nbad = int(differ.sum())
            print(f"{name} {m}x{n} bc={bc} k={k} three_chunks={three_chunks} strips={strips} chunks={chunks_i}/{chunks_e}: {nbad} of {differ.numel()} cells differ")
            assert nbad == 0, (name, dims, bc, k, three_chunks, nbad, tuple(int(x) for x in differ.nonzero()[0]))
        assert torch.equal(bits(u), bits(torch.from_numpy(host).cuda())), "the launch wrote its input"
