"""The shape of the plan each of the eight plan-creating entry points builds,
on a GPU: over one small layout that holds every tile kind (full and partial
vector tiles, a tail shorter than a vector, a lone scalar, an unaligned
tensor, an int64 segment; FA_PLAN_GAPS_ARE_PADDING), for the three element
types and both result types an entry accepts, the CPU order and the torch-GPU
order at n = 2, 5, 20 — every field of fa_plan_get_info, fa_plan_elem /
fa_plan_out_elem, and fa_plan_launch_shape / fa_plan_launch_form at n = 2, 5,
20, unweighted and weighted, equal to what the library built on an MI355X
before the entries were rebuilt over one constructor
(tests/golden/plan_shapes.json, tests/golden/make_plan_abi_golden.py)."""
import json
import os
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_plan_abi_golden as gold  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plans():
    """(recorded, built now): variant name -> record, every plan built once."""
    with open(gold.SHAPES) as f:
        want = json.load(f)["plans"]
    got = {f"{e}:{v}": gold.shape_record(e, a) for e, v, a in gold.shape_variants()}
    return want, got


def test_every_plan_is_built_as_the_parent_built_it(plans):
    want, got = plans
    assert sorted(want) == sorted(got) and len(want) == 51
    assert all(r["rc"] == 0 for r in want.values())
    bad = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not bad, list(bad.items())[:5]


def test_layout_holds_every_tile_kind(plans):
    """Two tile counts per entry family, scalar and vector tiles in each, and
    the three launch forms (batch, client loop, torch-GPU order)."""
    _, got = plans
    cpu, tgpu = got["fa_plan_create:f32/cpu"], got["fa_plan_create_order:f32/gpu5"]
    for r in (cpu, got["fa_plan_create_elem:bf16/cpu"]):
        i = r["info"]
        assert i["ntiles_cascade"] >= 3 and i["ntiles_tail"] >= 3 and i["tail_elems"] >= 4
        assert i["cascade_elems"] % i["tile_elems"] != 0     # a partial vector tile
    assert tgpu["info"]["tile_elems"] == 1024 and tgpu["launch"]["n5/w0"][1:] == [0, 0, 0, 0]
    assert cpu["launch"]["n20/w1"][3] == 16 and cpu["launch"]["n5/w0"][3] == 8
    assert got["fa_plan_create_elem:f16/cpu"]["launch"]["n5/w0"][3:] == [1, 1]


def test_forwarding_entries_build_the_same_plan(plans):
    """An _elem entry given FA_ELEM_F32 is the plain entry, an _elem_out entry
    with out_elem == elem the _elem entry, an _order* entry with the CPU order
    the entry without the order; fa_plan_create_from_tiles_elem over fp32 is
    fa_plan_create_from_tiles."""
    _, got = plans
    orders = ["cpu"] + [f"gpu{n}" for n in gold.SHAPE_N]
    same = [("fa_plan_create_elem:f32/cpu", "fa_plan_create:f32/cpu"),
            ("fa_plan_create_order:f32/cpu", "fa_plan_create:f32/cpu"),
            ("fa_plan_create_from_tiles_elem:f32/out_f32/cpu", "fa_plan_create_from_tiles:f32/cpu")]
    for o in orders:
        same.append((f"fa_plan_create_order_elem:f32/{o}", f"fa_plan_create_order:f32/{o}"))
    for e in ("f32", "f16", "bf16"):
        same.append((f"fa_plan_create_elem_out:{e}/out_{e}/cpu", f"fa_plan_create_elem:{e}/cpu"))
        same.append((f"fa_plan_create_order_elem:{e}/cpu", f"fa_plan_create_elem:{e}/cpu"))
        for o in orders:
            same.append((f"fa_plan_create_order_elem_out:{e}/out_{e}/{o}",
                         f"fa_plan_create_order_elem:{e}/{o}"))
    for e in ("f16", "bf16"):
        same.append((f"fa_plan_create_order_elem_out:{e}/out_f32/cpu",
                     f"fa_plan_create_elem_out:{e}/out_f32/cpu"))
    for a, b in same:
        assert got[a] == got[b], (a, b)
