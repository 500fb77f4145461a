"""CPU tests of the layout the workgroup-row 2D kernel's launcher chooses (lora_debug_wg_layout, no device): column strips of
512 - 6 (K - 1) output columns, row chunks of two classes (rim strips and the strips between them), all of them resident at
once where the launcher cuts the rows itself.

The planner scores a candidate by its predicted finish, max(interior steps, ratio x rim steps), a chunk of `rows` rows taking
rows + 7 K - 1 steps; the ratio is 1 + wg_edge_pct / 100, and the option's default is the measured cost of a rim-strip step
beside an interior one.  At 16384 x 16384, six applications, 256 CUs x 2 workgroups the 34 strips fill the 512
slots exactly with 32 x 15 + 2 x 16 chunks of 1134 and 1071 steps -- but only a ratio below 1218 / 1071 = 1.137 makes that layout
finish before the one with 14 interior chunks of 1218 steps; the test asserts the layout the shipped default implies and both layouts under explicit ratios.
"""
import ctypes

import numpy as np
import pytest

SHIPPED_EDGE_PCT = 12  # wg_edge_pct_default(6) (csrc/kernels_2d_wg.hip): a rim-strip workgroup finishes as if its steps cost 1.12 x the others'


@pytest.fixture(scope="module")
def L(engine_built):
    import lorastencil_amd as L

    return L


def layout(plan, k, rows, cus, per_cu):
    from lorastencil_amd import _lib

    out = (ctypes.c_int * 8)()
    rc = _lib.lib().lora_debug_wg_layout(plan._h, k, rows, cus, per_cu, out)
    assert rc == 0, rc
    return list(out)


def check(lay, k, rows, n, slots, one_round):
    strips, outw, rows_i, chunks_i, rows_e, chunks_e, wgs, rim = lay
    lag = 7 * k - 1
    assert outw == 512 - 6 * (k - 1)
    # strip s writes columns [s outw, min((s + 1) outw, n)): every column once exactly if the last strip is not empty
    assert (strips - 1) * outw < n <= strips * outw, lay
    assert rim == min(strips, 2), lay
    # chunk c of a strip writes rows [c rows_x, min((c + 1) rows_x, rows)): every row once exactly
    for between, r, c in ((True, rows_i, chunks_i), (False, rows_e, chunks_e)):
        if between and strips == rim:
            assert c == 0, lay
            continue
        assert r >= 1 and (c - 1) * r < rows <= c * r, lay
        assert (r + lag) % 7 == 0 and (r + lag) // 7 >= k + 1, lay  # whole groups of seven steps, every level started
    assert wgs == (strips - rim) * chunks_i + rim * chunks_e, lay
    if one_round and strips <= slots:
        assert wgs <= slots, (lay, slots)


def test_strips_and_chunks_cover_the_grid_once(L):
    rng = np.random.default_rng(20240607)
    n_cases = 0
    for _ in range(100):
        m = int(rng.choice([rng.integers(1, 200), rng.integers(200, 5000), rng.integers(5000, 40000)]))
        n = int(rng.choice([rng.integers(2, 600), rng.integers(600, 5000), rng.integers(5000, 40000)]))
        cus = int(rng.choice([8, 64, 256, 304]))
        per_cu = int(rng.choice([1, 2]))
        plan = L.Plan("star2d1r", (m, n))
        for k in (2, 4, 6):
            rows = m if rng.integers(0, 2) else int(rng.integers(1, m + 1))  # a launch over a share of the rows
            check(layout(plan, k, rows, cus, per_cu), k, rows, n, cus * per_cu, True)
            n_cases += 1
        plan.set_option("wg_edge_pct", int(rng.integers(0, 101)))
        check(layout(plan, 6, m, cus, per_cu), 6, m, n, cus * per_cu, True)
        plan.set_option("wg_rows", int(rng.integers(1, 2 * m + 2)))
        check(layout(plan, 4, m, cus, per_cu), 4, m, n, cus * per_cu, False)
        n_cases += 2
    assert n_cases == 500


def test_arguments(L):
    from lorastencil_amd import _lib

    lib = _lib.lib()
    out = (ctypes.c_int * 8)()
    p2, p1 = L.Plan("star2d1r", (64, 64)), L.Plan("1d1r", (4096,))
    assert lib.lora_debug_wg_layout(None, 6, 64, 256, 2, out) == _lib.LORA_EINVAL
    assert lib.lora_debug_wg_layout(p2._h, 6, 64, 256, 2, None) == _lib.LORA_EINVAL
    assert lib.lora_debug_wg_layout(p1._h, 6, 64, 256, 2, out) == _lib.LORA_EUNSUPPORTED
    for k, rows, cus, per_cu in ((3, 64, 256, 2), (8, 64, 256, 2), (6, 0, 256, 2), (6, 64, 0, 2), (6, 64, 256, 0)):
        assert lib.lora_debug_wg_layout(p2._h, k, rows, cus, per_cu, out) == _lib.LORA_EINVAL, (k, rows, cus, per_cu)


FULL_ROUND = [34, 482, 1093, 15, 1030, 16, 512, 2]  # 32 x 15 + 2 x 16 = 512 workgroups: 1134 and 1071 steps
FOURTEEN = (34, 482, 1177, 14)                     # 1218 steps in the strips between the rim strips


def test_the_flagship_layout(L):
    plan = L.Plan("star2d1r", (16384, 16384))
    lay = layout(plan, 6, 16384, 256, 2)
    check(lay, 6, 16384, 16384, 512, True)
    assert lay[0] == 34
    # 15 interior chunks leave the rim strips 16 chunks each: 1071 steps beside 1134.  Dearer rim steps finish last.
    full_round_pays = (100 + SHIPPED_EDGE_PCT) * 1071 < 100 * 1218
    if full_round_pays:
        assert lay == FULL_ROUND, lay
    else:
        assert tuple(lay[:4]) == FOURTEEN and lay[6] <= 512, lay
        assert (100 + SHIPPED_EDGE_PCT) * (lay[4] + 41) <= 100 * 1218, lay  # the rim chunks finish with the others
    # whatever the default: the two layouts under explicit ratios
    plan.set_option("wg_edge_pct", 5)
    assert layout(plan, 6, 16384, 256, 2) == FULL_ROUND
    plan.set_option("wg_edge_pct", 13)  # 1.13 x 1071 = 1210 < 1218: still ahead, by a hair
    assert layout(plan, 6, 16384, 256, 2) == FULL_ROUND
    plan.set_option("wg_edge_pct", 14)
    assert tuple(layout(plan, 6, 16384, 256, 2)[:4]) == FOURTEEN
    plan.set_option("wg_edge_pct", 60)
    lay = layout(plan, 6, 16384, 256, 2)
    check(lay, 6, 16384, 16384, 512, True)
    assert tuple(lay[:4]) == FOURTEEN and 160 * (lay[4] + 41) <= 100 * 1218, lay
