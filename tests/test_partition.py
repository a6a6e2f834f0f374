import pytest

from conftest import load_manifest
from feddct_amd.layout import BucketLayout
from feddct_amd.partition import i64_tiles, layout_tiles, split_tiles


@pytest.mark.parametrize("lay", ["wrn16_8_c10", "wrnsl16_8_sf4_c100_proxy", "wrnsl16_8_sf4_c10_main"])
@pytest.mark.parametrize("parts", [1, 2, 3, 8, 100])
def test_split_covers_every_tile_once(lay, parts):
    L = BucketLayout.from_manifest(load_manifest(lay))
    info, tiles = layout_tiles(L)
    sp = split_tiles(tiles, parts, L.f32_numel)
    assert len(sp) == parts
    assert sp[0][0] == 0 and sp[-1][1] == L.f32_numel
    n = 0
    for (lo, hi, sel), nxt in zip(sp, sp[1:] + [(L.f32_numel, None, None)]):
        assert hi == nxt[0] and lo <= hi and lo % 4 == 0
        if len(sel):
            assert (sel[:, 0] >= lo).all() and ((sel[:, 0] + sel[:, 1]) <= hi).all()
        n += len(sel)
    assert n + len(i64_tiles(tiles)) == len(tiles)
    if parts <= 8 and lay != "wrnsl16_8_sf4_c10_main":
        sizes = [int(sel[:, 1].sum()) if len(sel) else 0 for _, _, sel in sp]
        assert max(sizes) < 2.5 * (sum(sizes) / parts) + 4096


@pytest.mark.parametrize("lay", ["wrn16_8_c10", "wrnsl16_8_sf4_c100_proxy"])
def test_split_by_fractions_tapers(lay):
    """pipeline.HostPipeline's tapered cut: every tile once, each range near
    its fraction of the elements (cuts fall on tile starts)."""
    fr = (0.5, 0.25, 0.125, 0.0625, 0.0625)
    L = BucketLayout.from_manifest(load_manifest(lay))
    info, tiles = layout_tiles(L)
    sp = split_tiles(tiles, len(fr), L.f32_numel, fr)
    assert sp[0][0] == 0 and sp[-1][1] == L.f32_numel
    assert sum(len(sel) for _, _, sel in sp) + len(i64_tiles(tiles)) == len(tiles)
    sizes = [int(sel[:, 1].sum()) for _, _, sel in sp]
    total = sum(sizes)
    for got, want in zip(sizes, fr):
        assert abs(got / total - want) < 0.03, (sizes, fr)
    with pytest.raises(ValueError):
        split_tiles(tiles, 3, L.f32_numel, fr)


# ------------------------------ the host-resident round's test layouts --
@pytest.mark.parametrize("cut", ["taper", "taper_nb", "even6", "even64"])
@pytest.mark.parametrize("lay", ["mid", "tiny", "onetile", "noi64", "nof32", "sweep"])
def test_host_round_layout_cuts(lay, cut):
    """The cuts pipeline.HostPipeline makes of the layouts that
    test_gpu_host_round.py runs (hostlayouts.py): the ranges cover
    [0, f32_numel) exactly and in order, every range starts 16-B aligned,
    every fp32 tile is in exactly one range and lies inside it, and the number
    of non-empty ranges is the one those tests rely on."""
    import hostlayouts as H
    man = H.SWEEP if lay == "sweep" else H.LAYOUTS[lay]
    L, tiles, sp = H.cut(man, cut, H.SWEEP_TILE if lay == "sweep" else 0)
    parts = H.CUTS[cut][0]
    assert len(sp) == parts
    assert sp[0][0] == 0 and sp[-1][1] == L.f32_numel
    t32 = tiles[tiles[:, 2] < 4]
    seen = 0
    for (lo, hi, sel), nxt in zip(sp, sp[1:] + [(L.f32_numel, None, None)]):
        assert hi == nxt[0] and lo <= hi and lo % 4 == 0
        assert (hi > lo) == (len(sel) > 0)       # a range is empty iff it has no tile
        if len(sel):
            assert (sel[:, 0] >= lo).all() and ((sel[:, 0] + sel[:, 1]) <= hi).all()
        seen += len(sel)
    assert seen == len(t32) and seen + len(i64_tiles(tiles)) == len(tiles)
    # no tile twice: the selected starts are the table's, each once
    starts = sorted(int(s) for _, _, sel in sp for s in sel[:, 0])
    assert starts == sorted(int(s) for s in t32[:, 0])
    nonempty = sum(hi > lo for lo, hi, _ in sp)
    assert nonempty == H.NONEMPTY[lay][cut], (lay, cut, nonempty)


def test_host_round_layout_facts():
    """The figures the host-round tests quote for their layouts."""
    import hostlayouts as H
    L, tiles, sp = H.cut(H.LAYOUTS["mid"], "taper")
    t32 = tiles[tiles[:, 2] < 4]
    assert L.f32_numel == 133504 and L.i64_numel == 2
    assert len(t32) == 74 and int((t32[:, 2] == 0).sum()) == 68
    assert [int(sel[:, 1].sum()) for _, _, sel in sp] == H.MID_TAPER_SIZES
    L, tiles, sp = H.cut(H.LAYOUTS["tiny"], "even64")
    assert [hi - lo for lo, hi, _ in sp[1:]] == [0] * 63
    L, tiles, sp = H.cut(H.LAYOUTS["onetile"], "taper")
    t32 = tiles[tiles[:, 2] < 4]
    assert len(t32) == 1 and int(t32[0, 2]) == 0 and int(t32[0, 1]) == 2048
    L, tiles, sp = H.cut(H.LAYOUTS["noi64"], "taper")
    assert L.i64_numel == 0 and len(i64_tiles(tiles)) == 0
    assert sum(hi == lo for lo, hi, _ in sp) == 3
    L, tiles, sp = H.cut(H.LAYOUTS["nof32"], "taper")
    assert L.f32_numel == 0 and all((lo, hi) == (0, 0) and len(sel) == 0 for lo, hi, sel in sp)
    assert len(i64_tiles(tiles)) >= 1
    # the sweep's layout: about 40 tiles of 1024, five taper ranges, and
    # N = 300 pinned rows of it stay under 64 MB
    L, tiles, sp = H.cut(H.SWEEP, "taper", H.SWEEP_TILE)
    t32 = tiles[tiles[:, 2] < 4]
    assert 40 <= len(t32) <= 64 and int(t32[:, 1].max()) <= 1024
    assert (t32[:, 2] != 0).sum() >= 4           # scalar tails among them
    assert 300 * (4 * max(L.f32_numel, 64) + 8 * L.i64_numel) < 64 << 20
    # a cut with more parts than tiles: empty ranges, every tile still once
    L, tiles, _ = H.cut(H.LAYOUTS["mid"], "taper")
    sp = split_tiles(tiles, 200, L.f32_numel)
    assert sum(len(sel) for _, _, sel in sp) == 74
    assert sum(hi == lo for lo, hi, _ in sp) >= 200 - 74
