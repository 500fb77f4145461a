"""The workgroup-row 2D kernel (kernels_2d_wg.hip) keeps, per level whose producer is the same wave, the pair a lane published
one step ago in registers instead of reading it back from the level's LDS row (its window is then three pieces, not four),
sets its EDGE-only masks up once per EDGE range of groups, and in interior steps of the nested-profile form fetches the next
level's window while the current level's scatter multiply-adds issue.  None of it may change a bit of the result.

Every case compares ONE launch of 6, 4 or 2 applications (lora_plan_stepn_region) BIT FOR BIT, over the whole padded buffer,
with the same number of single sweeps of a steps_per_launch = 1 plan driven as lora_plan_run's step-by-step loop drives them:
buffer 0 carries the caller's halo, buffer 1's halo is zero (reference boundary) or a copy of buffer 0's (Dirichlet option).

Sizes (rows x columns; strips are 476 / 488 / 500 output columns at 6 / 4 / 2 applications):
  97 x 953     every strip sees columns outside the interior in every step (EDGE throughout); the odd extent leaves the last
               column pair half valid
  300 x 1500   strips that never see a column outside the interior between two rim strips; with one chunk per strip
               (wg_rows) that chunk runs EDGE groups, interior groups and EDGE groups again: the carried pairs cross both
               changes of loop and the masks are set up twice
  2100 x 1500  several chunks per strip: the inner chunks run interior groups only, dozens of 7-step groups of them
Each size runs with the launch's own chunk rule and with one chunk per interior strip.  Under the Dirichlet option a grid with
an odd innermost extent has no fused launch at all (its plan runs the generic kernel): at 97 x 953 those cases check the
refusal, and 97 x 954 runs the Dirichlet launches of a grid whose strips are all rim strips.

Taps: star2d1r (nested-profile evaluation), box2d3r (the form its plan resolves) and a full-rank 49-tap table (the taps one by
one).  Inputs: seeded integers 0..99 -- sums stay exact, so a structured form of the fused launch and the direct taps of the
single sweeps agree to the bit -- and, for the 49-tap table, whose fused and single-sweep kernels apply the taps in the same
order, seeded normal doubles, where every rounding counts.  The one combination whose sums are NOT exact -- box2d3r in its
pyramid form at six applications, past 2^53 -- is compared bit for bit with the row-streaming kernel in the same form and,
with the taps one by one, with the single sweeps (see the comment in the test).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [(97, 953), (300, 1500), (2100, 1500)]
# (id, shape, full-rank table?, input, boundary, depths of the launches)
CASES = [
    ("star2d1r", "star2d1r", False, "int", "reference", (6, 4, 2)),
    ("box2d3r", "box2d3r", False, "int", "reference", (6, 4, 2)),
    ("taps49", "box2d3r", True, "int", "reference", (6, 4, 2)),
    ("taps49_normal", "box2d3r", True, "normal", "reference", (6, 4, 2)),
    # the Dirichlet option runs this kernel at four and two applications, for tables with a structured form
    ("star2d1r_dirichlet", "star2d1r", False, "int", "dirichlet", (4, 2)),
    ("box2d3r_dirichlet", "box2d3r", False, "int", "dirichlet", (4, 2)),
]


@pytest.fixture(scope="module")
def L(engine_built):
    import torch

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    import lorastencil_amd as L

    assert L.device_count() >= 1
    return L


def taps49():
    """full rank, dyadic (as test_gpu_memory_contract.py): no structured form, exact sums on small integers"""
    return np.random.default_rng(49).integers(-2, 3, 49).astype(np.float64) / 64.0


def bits(t):
    import torch

    return t.view(torch.int64)


# every case at every size; the Dirichlet cases also at 97 x 954: the even twin of 97 x 953, where they have no launch
PARAMS = [(c, d) for c in CASES for d in SIZES + ([(97, 954)] if c[4] == "dirichlet" else [])]


@pytest.mark.parametrize("case,dims", PARAMS, ids=[f"{c[0]}-{d[0]}x{d[1]}" for c, d in PARAMS])
def test_fused_launch_is_the_single_sweeps_bit_for_bit(L, case, dims):
    import torch

    name, shape, full_rank, kind, bc, depths = case
    m, n = dims
    if bc == "dirichlet" and n % 2:
        # No such launch exists: under the Dirichlet option a grid with an odd innermost extent runs single sweeps of the
        # generic kernel (plan.cpp), and its plan refuses every fused depth.  That is all there is to check at this size;
        # 97 x 954 below runs the Dirichlet launches of a grid whose strips are all rim strips.
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

    # the step-by-step driver, once: level k of it for every depth compared below
    single = L.Plan(shape, dims).set_option("steps_per_launch", 1)
    if full_rank:
        single.set_weights(taps49())
    assert single.get_option("steps_per_launch") == 1 and "wg" not in single.kernel_name
    buf = [u.clone(), torch.zeros_like(u)]
    if bc == "dirichlet":
        single.halo(buf[1], "copy", buf[0])
    want = {}
    for k in range(1, max(depths) + 1):
        single.step(buf[(k - 1) % 2], buf[k % 2])
        if k in depths:
            want[k] = buf[k % 2].clone()  # (even k: buffer 0, whose halo is the caller's)
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(w).all()) for w in want.values())

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

    def same(got, ref, what):
        differ = bits(got) != bits(ref)
        nbad = int(differ.sum())
        print(f"{name} {m}x{n} bc={bc} {what}: {nbad} of {differ.numel()} cells differ")
        assert nbad == 0, (name, dims, bc, what, nbad, tuple(int(x) for x in differ.nonzero()[0]))

    # A structured form of the fused launch (pyramid, nested profiles) sums the same products in another order than the
    # direct taps of a single sweep: the two agree to the bit exactly while no partial sum needs rounding, that is while
    # 99 (sum |w|)^k < 2^53 (integer taps on integers 0..99).  box2d3r's taps sum to 232: six sweeps reach 1.5e16 > 2^53 =
    # 9.0e15 (measured: 2 of 464464 cells of 300 x 1500 differ from the single sweeps in the last bit).  For such a depth
    # the launch in its own form is compared, bit for bit, with the row-streaming kernel (kernels_2d_stream.hip) in the
    # SAME form -- four applications, then two: the taps reach every accumulator in the same order in both kernels -- and
    # the launch with the taps one by one (lowrank_valu = 0: the single sweeps' own order) with the single sweeps.
    wsum = float(np.abs(make({}).weights).sum())
    for one_chunk in (False, True):
        geometry = {"wg_rows": m} if one_chunk else {}
        plan = make(geometry)
        sig = plan.kernel_signature
        assert plan.kernel_name == "stencil2d_wg_kernel", sig
        assert plan.get_option("steps_per_launch") == max(depths), sig
        assert ("eval=7" in sig) == (shape == "star2d1r") and (not full_rank or "eval=2" in sig), sig
        structured = not any(f"eval={e}," in sig for e in (0, 1, 2))
        for k in depths:
            what = f"k={k} one_chunk={one_chunk} [{sig}]"
            if kind == "normal" or not structured or 99.0 * wsum ** k < 2.0 ** 53:
                same(launch(plan, k, u), want[k], what)
                continue
            assert k == 6 and bc == "reference"
            s4, s2 = make({"steps_per_launch": 4}), make({"steps_per_launch": 2})
            form = sig[sig.index("eval="):sig.index(",")]
            for s in (s4, s2):
                assert s.kernel_name == "stencil2d_stream_kernel" and form + "," in s.kernel_signature, s.kernel_signature
            same(launch(plan, 6, u), launch(s2, 2, launch(s4, 4, u)), what + " against the row-streaming kernel, 4 + 2")
            direct = make(dict(geometry, lowrank_valu=0))
            assert direct.kernel_name == "stencil2d_wg_kernel" and "eval=2," in direct.kernel_signature
            same(launch(direct, 6, u), want[6], f"k=6 one_chunk={one_chunk} [{direct.kernel_signature}]")
        assert torch.equal(bits(u), bits(torch.from_numpy(host).cuda())), "the launch wrote its input"
