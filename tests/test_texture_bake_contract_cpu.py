"""CPU: the contract of the texture-atlas kernels (csrc/texture_bake_core.h).  The host emulation built from the header against a numpy
restatement written from the contract's text, every byte; the atlas layout at its edges, and that the four texels the rasteriser's
bilinear fetch reads for any point of a triangle are texels of that triangle's own chart; the accuracy of the baked colour against the
analytic colour the views were painted with.  No GPU, no engine library."""
import functools
import math

import numpy as np
import pytest

from tests.support import texture_bake as tb


@functools.lru_cache(None)
def _restated64():
    """the float64 restatement of the bake of the accuracy test, once"""
    v, f, _ = tb.ico_mesh()
    return tb.restated_bake(v, f, tb.sphere_views(), 512, dt=np.float64, details=True)


@pytest.mark.parametrize("S,B", [(256, 8), (512, 16)])
@pytest.mark.parametrize("best_view", [False, True])
def test_emulation_equals_the_restatement(S, B, best_view):
    v, f, colors = tb.ico_mesh()
    views = tb.sphere_views()
    assert len(f) == 1280 and tb.emul_block(len(f), S) == B == tb.restated_block(len(f), S)
    for masks in (True, False):
        for cols in (colors, None):
            got = tb.emul_bake(v, f, views, S, colors=cols, masks=masks, best_view=best_view)
            want = tb.restated_bake(v, f, views, S, colors=cols, masks=masks, best_view=best_view)
            for a, b, name in zip(got, want, ("texels", "seen")):
                assert a.dtype == b.dtype and a.shape == b.shape
                assert np.array_equal(a, b), (masks, cols is not None, name, int((a != b).sum()))
            texels, seen = got
            assert seen.max() >= 2 and (seen == 0).any() and (texels[..., 3] == 255).sum() > 0.6 * S * S
    assert np.array_equal(tb.emul_uvs(len(f), S), tb.restated_uvs(len(f), S))


def test_the_modes_and_inputs_differ_where_they_should():
    """blend and best_view, masks, and the fallback colours each change bytes: none of the comparisons above is between two ignored inputs"""
    v, f, colors = tb.ico_mesh()
    views = tb.sphere_views()
    blend, seen = tb.emul_bake(v, f, views, 256, colors=colors)
    best, seen_b = tb.emul_bake(v, f, views, 256, colors=colors, best_view=True)
    assert np.array_equal(seen, seen_b) and (blend != best).any()
    white, _ = tb.emul_bake(v, f, views, 256)
    unseen = (seen == 0) & (blend[..., 3] == 255)
    assert unseen.any() and (white[unseen][:, :3] == 255).all() and (blend[unseen][:, :3] != 255).any()
    assert np.array_equal(white[seen > 0], blend[seen > 0])
    holes = dict(views)
    holes["masks"] = views["masks"].copy()
    holes["masks"][:, ::2, ::2] = 0                          # with masks: no four taps pass any more
    masked, seen_m = tb.emul_bake(v, f, holes, 256, colors=colors)
    assert (seen_m < seen).any() and (masked != blend).any()
    assert np.array_equal(tb.emul_bake(v, f, holes, 256, colors=colors, masks=False)[0], tb.emul_bake(v, f, views, 256, colors=colors, masks=False)[0])


def test_atlas_block_at_its_edges():
    for fn in (tb.emul_block, tb.restated_block):
        assert [fn(T, 64) for T in (1, 2, 3)] == [64, 64, 32]
        assert fn(8, 64) == 32 and fn(9, 64) == 16                     # exactly full, one too many
        assert fn(32, 64) == 16 and fn(33, 64) == 8
        assert fn(512, 64) == 4 and fn(513, 64) == 0                   # too many for B = 4
        assert fn(2 * 2048 * 2048, 8192) == 4 and fn(2 * 2048 * 2048 + 1, 8192) == 0
        assert fn(1280, 256) == 8 and fn(1280, 512) == 16
    assert tb.emul_block(0, 64) == 0 and tb.emul_block(-1, 64) == 0
    for S in (0, 32, 96, 100, 16384):                                  # not a power of two in 64 .. 8192
        assert tb.emul_block(2, S) == 0


@pytest.mark.parametrize("T,S,B", [(80, 64, 8), (320, 64, 4), (7, 64, 32), (1, 64, 64), (1280, 256, 8)])
def test_the_rasterisers_taps_stay_inside_the_triangles_own_chart(T, S, B):
    """tex_sample at level 0, restated on integers: for the corners, the edge midpoints and a few hundred points inside every triangle,
    the four texels it reads are texels the bake assigned to that triangle.  A tap whose bilinear weight is below 2^-16 may be exempt
    (rounding of the UV at a corner or an edge puts the sample a hair outside); none is for a point strictly inside."""
    assert tb.emul_block(T, S) == B
    uvs = tb.emul_uvs(T, S)
    assert np.array_equal(uvs, tb.restated_uvs(T, S))
    _, owner, _, _, _ = tb.chart_texels(T, S)
    rng = np.random.default_rng(5)
    inner = rng.dirichlet((1.0, 1.0, 1.0), 300) * 0.97 + 0.01          # every weight at least 0.01
    grid = np.array([(i, j, 12 - i - j) for i in range(1, 12) for j in range(1, 12 - i)], np.float64) / 12.0
    edge = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (.5, .5, 0), (0, .5, .5), (.5, 0, .5), (.25, .75, 0), (0, .125, .875), (.999, 0, .001)])
    exempt_total = 0
    for name, bary in (("inside", np.concatenate([inner, grid])), ("boundary", edge)):
        w = bary.astype(np.float32)
        uv = (w[None, :, 0, None] * uvs[:, None, 0] + w[None, :, 1, None] * uvs[:, None, 1]) + w[None, :, 2, None] * uvs[:, None, 2]   # [T,P,2]
        assert uv.dtype == np.float32
        x, y, wgt = tb.level0_taps(uv[..., 0].reshape(-1), uv[..., 1].reshape(-1), S)
        want = np.repeat(np.arange(T), len(bary))[:, None]
        foreign = owner[y, x] != want
        exempt = foreign & (wgt < 2.0 ** -16)
        assert not (foreign & ~exempt).any(), (name, int((foreign & ~exempt).sum()))
        print(f"T {T} S {S} B {B} {name}: {x.size} taps, {int(exempt.sum())} exempt")
        if name == "inside":
            assert not exempt.any()
        exempt_total += int(exempt.sum())
    assert exempt_total <= 4 * len(edge) * T


def test_corner_texels_bake_the_corners_and_gutters_the_hypotenuse():
    """the chart coordinates: (0,0), (1,0), (0,1) at the corner texels of both charts, a + b = 1 on the spill and gutter diagonals"""
    for T, S in ((2, 64), (320, 64), (1280, 256)):
        B = tb.restated_block(T, S)
        c = B - 3
        t, a, b = tb.chart_coordinates(T, S)
        assert (a >= 0).all() and (b >= 0).all() and (a + b <= 1 + 1e-6).all()
        assert (a[0, 0], b[0, 0]) == (0, 0) and (a[0, c], b[0, c]) == (1, 0) and (a[c, 0], b[c, 0]) == (0, 1) and t[0, 0] == 0
        assert (a[B - 1, B - 1], b[B - 1, B - 1]) == (0, 0) and (a[B - 1, B - 1 - c], b[B - 1, B - 1 - c]) == (1, 0) and t[B - 1, B - 1] == 1
        assert (a[B - 1 - c, B - 1], b[B - 1 - c, B - 1]) == (0, 1)
        j, i = np.mgrid[0:B, 0:B]
        for d, tri in ((B - 2, 0), (B - 1, 0), (B, 1)):
            on = (i + j) == d
            assert (t[:B, :B][on] == tri).all() and np.allclose((a + b)[:B, :B][on], 1.0, atol=1e-6)


# the float64 restatement's largest difference to the analytic colour, measured, and the bound the test holds the emulation to
F64_MAX_DIFF = 4.245
BOUND = 7


def test_baked_colour_against_the_analytic_colour():
    """The icosphere (1 280 faces, S = 512, B = 16) under the eight corner cameras of the sphere's views, whose pixels are painted with
    128 + 2000 p of the sphere's surface point p (cut to a byte).  Every seen texel's byte against that function at the texel's own
    surface point.  Condition: at least 95 % of the chart texels are seen at cos_min = 0.2 -- the float64 restatement alone is
    checked for it first.
    MEASURED: the float64 restatement's largest |difference| before quantising is F64_MAX_DIFF = 4.245 levels (mean 0.53; 99.99 % of
    the 163 840 chart texels seen), so BOUND = ceil(1.5 x 4.245) = 7 levels, which the fp32 emulation's bytes must meet (they reach
    4.245, mean 0.56).  The largest differences are at texels that four views see, each at cos 0.46 .. 0.51 (the points farthest from
    every camera); the views' bytes are cut, not rounded, which alone is half a level."""
    v, f, _ = tb.ico_mesh()
    texels64, seen64, det = _restated64()
    chart = det["t"] >= 0
    share = float((seen64[chart] > 0).mean())
    want = tb.analytic_rgb(det["p"])
    diff64 = np.abs(det["raw"] - want)[chart & (seen64 > 0)]
    print(f"seen {share:.4f} of {int(chart.sum())} chart texels; float64 restatement: max |diff| {diff64.max():.3f}, mean {diff64.mean():.3f} levels")
    assert share >= 0.95
    texels, seen = tb.emul_bake(v, f, tb.sphere_views(), 512)
    assert np.array_equal(seen, seen64) or float((seen != seen64).mean()) < 1e-3      # a texel on the edge of a test may flip in fp32
    both = chart & (seen > 0)
    diff = np.abs(texels[..., :3].astype(np.float64) - want)[both]
    print(f"fp32 emulation: max |diff| {diff.max():.3f}, mean {diff.mean():.3f} levels; bound {BOUND}")
    assert abs(diff64.max() - F64_MAX_DIFF) < 2e-3 and math.ceil(1.5 * F64_MAX_DIFF) == BOUND, "the documented measurement is stale"
    assert diff.max() <= BOUND
