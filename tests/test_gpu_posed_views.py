"""GPU: the one marshaller of a set of posed views (engine._posed_views) through the three entries that use it -- tsdf_integrate,
tsdf_track and texture_bake -- on a 4 x 4 x 4 volume, a one-triangle mesh in a 64-texel atlas and two views of 4 x 6: a malformed
depth, K, masks or rgb is refused by every entry with the same text, poses of [n,3,4] are taken by integrate and bake (and give the
bits of [n,4,4]) and refused by track, and no view at all returns what it always returned.  Reads nothing outside the tree."""
import pytest
import torch

pytestmark = pytest.mark.gpu
ORIGIN, VOXEL, SIZE = (-0.03, -0.03, -0.03), 0.02, 64


def _views():
    depth = torch.full((2, 4, 6), 0.5, device="cuda")
    K = torch.tensor([[10.0, 0.0, 3.0], [0.0, 10.0, 2.0], [0.0, 0.0, 1.0]], device="cuda").repeat(2, 1, 1)
    TCO = torch.eye(4, device="cuda").repeat(2, 1, 1)
    TCO[:, 2, 3] = 0.5
    TCO[1, 0, 3] = 0.01
    return dict(depth=depth, K=K, TCO=TCO, masks=torch.ones(2, 4, 6, dtype=torch.uint8, device="cuda"),
                rgb=torch.full((2, 4, 6, 3), 128, dtype=torch.uint8, device="cuda"))


def _entries():
    """name -> (call(**views), takes rgb); every call starts from an empty volume"""
    from megapose6d_amd import engine as eng

    v = torch.tensor([[-0.02, -0.02, 0.0], [0.02, -0.02, 0.0], [0.0, 0.02, 0.0]], device="cuda")
    f = torch.tensor([[0, 2, 1]], dtype=torch.int32, device="cuda")          # the normal is -z: towards both cameras

    def integrate(depth, K, TCO, masks, rgb):
        vol = eng.tsdf_volume((4, 4, 4), True, "cuda")
        assert eng.tsdf_integrate(vol, ORIGIN, VOXEL, depth, K, TCO, masks=masks, rgb=rgb) is None
        return vol

    def track(depth, K, TCO, masks, rgb):
        return eng.tsdf_track(eng.tsdf_volume((4, 4, 4), True, "cuda"), ORIGIN, VOXEL, depth, K, TCO, masks=masks, iters=1)

    def bake(depth, K, TCO, masks, rgb):
        return eng.texture_bake(v, f, depth, K, TCO, masks, rgb, SIZE, depth_tol=0.01)

    return dict(integrate=(integrate, True), track=(track, False), bake=(bake, True))


def _refusal(call, views, **bad):
    from megapose6d_amd import engine as eng

    with pytest.raises(eng.EngineError) as e:
        call(**{**views, **bad})
    return str(e.value)


def test_every_entry_refuses_a_malformed_view_set_with_the_same_text():
    views, entries = _views(), _entries()
    for bad, text, needs_rgb in ((dict(depth=views["depth"][0]), "depth must be [n,h,w], got (4, 6)", False),
                                 (dict(K=views["K"][:, :2]), "K must be [n,3,3], got (2, 2, 3)", False),
                                 (dict(masks=views["masks"][:, :3]), "masks must be (2, 4, 6), got (2, 3, 6)", False),
                                 (dict(rgb=views["rgb"][:, :, :5]), "rgb must be (2, 4, 6, 3), got (2, 4, 5, 3)", True)):
        for name, (call, takes_rgb) in entries.items():
            if takes_rgb or not needs_rgb:
                assert _refusal(call, views, **bad) == text, (name, bad.keys())


def test_poses_of_three_rows_are_taken_by_integrate_and_bake_and_refused_by_track():
    views, entries = _views(), _entries()
    rows3 = views["TCO"][:, :3].contiguous()
    for name in ("integrate", "bake"):
        got, want = entries[name][0](**{**views, "TCO": rows3}), entries[name][0](**views)
        for a, b in zip(got if isinstance(got, tuple) else (got,), want if isinstance(want, tuple) else (want,)):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), name
    assert bool(entries["integrate"][0](**views)[1].view(torch.int32).any()) and bool(entries["bake"][0](**views)[1].any())   # something was seen
    assert _refusal(entries["track"][0], views, TCO=rows3) == "TCO must be [n,4,4], got (2, 3, 4)"
    assert [tuple(t.shape) for t in entries["track"][0](**views)] == [(2, 4, 4), (2,), (2,), (2,)]


def test_no_view_at_all_returns_what_it_returned():
    views, entries = _views(), _entries()
    none = {k: t[:0] for k, t in views.items()}
    assert not bool(entries["integrate"][0](**none).view(torch.int32).any())                    # a no-op
    assert [tuple(t.shape) for t in entries["track"][0](**none)] == [(0, 4, 4), (0,), (0,), (0,)]
    texels, seen = entries["bake"][0](**none)
    chart = texels[..., 3] == 255
    assert bool(chart.any()) and bool((texels[chart] == 255).all()) and not bool(texels[~chart].any()) and not bool(seen.any())   # white charts
