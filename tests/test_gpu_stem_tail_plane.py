"""-m gpu: the stem's tail-plane walks (csrc/conv_stem.hip, TAIL instances; mp_conv_stem_xrec_tail).

A walk whose last real record element sits alone in its 16-byte chunk leaves that chunk out of the per-tap slices and takes the element
from a plane in LDS (one K slice per kernel row): the dense walk of the RGB refiner's record (33 real elements: 62 -> 52 steps at 7x7)
and the background walk of every record with three crop channels (9 pieces: 26 -> 14 steps; new for the coarse net's 16 elements).
Shapes are the smallest at which the walk can go wrong: one 8 x 16 output tile (16 x 32 input) and a ragged second tile row and column
(18 x 34: plane entries at the right and bottom image edge), one and two channel blocks, with and without the fused max pool.
  * against a float64 direct convolution of the decoded records, 2e-5 of the output scale;
  * one-hot inputs and weights: a wrong tap-to-weight mapping of the tail slices (or of the first main element) is an O(1) error;
  * the background walk against the dense walk on inputs without renders: <= 2e-6 of the output scale, bit-identical when every flag
    says "geometry";
  * MP_STEM_TAIL=0 gives the outputs of the commit before the tail plane, bit for bit (tests/golden/stem_tail_switch_parent.npz).
"""
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "stem_tail_switch_parent.npz"


@pytest.fixture(scope="module")
def eng():
    from megapose6d_amd import engine

    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return engine


def split3(v: torch.Tensor):
    """exact truncation split of fp32 values into three bf16-representable fp32 pieces"""
    def trunc(t):
        return (t.view(torch.int32) & -65536).view(torch.float32)
    h = trunc(v)
    r = v - h
    m = trunc(r)
    return h, m, r - m


def to_records(eng, x_nchw: torch.Tensor, nf: int, border: int) -> torch.Tensor:
    """fp32 [n, c, h, w] (CPU) -> bf16 record tensor on the device: three exact pieces of the first `nf` channels, then k of k / 255"""
    n, c, h, w = x_nchw.shape
    R = eng.xrec_elements(nf, c - nf)
    buf = eng.padded_nhwc(n, h, w, R, border, "cuda", dtype=torch.bfloat16)
    v = eng.padded_view(buf, n, h, w, R, border)
    xl = x_nchw.permute(0, 2, 3, 1).contiguous()
    k = torch.round(xl[..., nf:] * 255.0)
    assert torch.equal(k / 255.0, xl[..., nf:])
    pieces = torch.stack(split3(xl[..., :nf].contiguous()), dim=-1).reshape(n, h, w, 3 * nf)
    v[..., : 3 * nf] = pieces.cuda().to(torch.bfloat16)
    v[..., 3 * nf : c + 2 * nf] = k.cuda().to(torch.bfloat16)
    assert torch.equal(v[..., : 3 * nf].float().cpu(), pieces)
    return buf


def tile_flags_of(x_nchw: torch.Tensor, nf: int) -> torch.Tensor:
    """one byte per (image, 8x8-pixel tile): does any integer channel of the tile hold a non-zero value (what the rasteriser reports)"""
    n, c, h, w = x_nchw.shape
    any_px = (x_nchw[:, nf:] != 0).any(dim=1)
    padded = torch.zeros(n, (h + 7) // 8 * 8, (w + 7) // 8 * 8, dtype=torch.bool)
    padded[:, :h, :w] = any_px
    return padded.view(n, (h + 7) // 8, 8, (w + 7) // 8, 8).any(dim=4).any(dim=2).to(torch.uint8).cuda().contiguous()


class Stem:
    """one stem layer with the blobs of its tail-plane forms; run() returns (stem map, pooled map) of one launch"""

    def __init__(self, eng, x, nf, K, w, scale, bias, relu=True, rec=None):
        self.eng, self.nf, self.K, self.relu = eng, nf, K, relu
        self.N, self.C, self.H, self.W = x.shape
        self.Cout = w.shape[0]
        self.pad = K // 2
        self.Ho, self.Wo = (self.H + 2 * self.pad - K) // 2 + 1, (self.W + 2 * self.pad - K) // 2 + 1
        self.Hq, self.Wq = (self.Ho - 1) // 2 + 1, (self.Wo - 1) // 2 + 1
        self.rec = to_records(eng, x, nf, self.pad) if rec is None else rec
        self.bias = bias.cuda()
        self.forms = eng.conv_stem_tail_forms(K, nf, self.C - nf)
        wn, sn = w.numpy(), scale.numpy()
        self.w_dense = torch.from_numpy(eng.conv_stem_pack_weights_tail(wn, nf, sn) if self.forms & 1 else eng.conv_stem_pack_weights(wn, nf, sn)).cuda()
        self.w_bg = torch.from_numpy(eng.conv_stem_pack_weights_tail(wn, nf, sn, background=True)).cuda() if self.forms & 2 else None
        ref = F.conv2d(x.double(), (w * scale.view(-1, 1, 1, 1)).double(), bias.double(), stride=2, padding=self.pad)
        self.ref = F.relu(ref) if relu else ref
        self.scale = max(1.0, self.ref.abs().max().item())

    def run(self, pool, flags=None):
        e = self.eng
        y = e.padded_nhwc(self.N, self.Ho, self.Wo, self.Cout, 1, "cuda")
        e.padded_view(y, self.N, self.Ho, self.Wo, self.Cout, 1)[:] = 7.0     # poison: the interior must be overwritten
        q = None
        if pool:
            q = e.padded_nhwc(self.N, self.Hq, self.Wq, self.Cout, 1, "cuda")
            e.padded_view(q, self.N, self.Hq, self.Wq, self.Cout, 1)[:] = 7.0
        sp = flags is not None
        e.conv_stem_xrec(self.rec, self.N, self.H, self.W, self.C, self.nf, self.pad, self.w_dense, self.bias, self.Cout, self.K, self.pad, y, 1,
                         relu=self.relu, y_pool=q, pool_border=1, w_sparse=self.w_bg if sp else None, tile_flags=flags if sp else None,
                         tail_forms=self.forms)   # (without flags only bit 0 matters: the instance is the same, every workgroup walks dense)
        torch.cuda.synchronize()
        return y, q

    def nchw(self, y):
        return self.eng.padded_view(y, self.N, self.Ho, self.Wo, self.Cout, 1).permute(0, 3, 1, 2).cpu().double()

    def pooled_nchw(self, q):
        return self.eng.padded_view(q, self.N, self.Hq, self.Wq, self.Cout, 1).permute(0, 3, 1, 2).cpu().double()


def make_layer(K, nf, nu, H, W, Cout, seed, N=2, renders=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.cat([torch.randn(N, nf, H, W, generator=g) * 0.3 + 0.5, torch.randint(0, 256, (N, nu, H, W), generator=g).float() / 255.0], dim=1)
    if not renders:
        x[:, nf:] = 0.0
    w = torch.randn(Cout, nf + nu, K, K, generator=g) * (2.0 / ((nf + nu) * K * K)) ** 0.5
    scale, bias = torch.rand(Cout, generator=g) + 0.5, torch.randn(Cout, generator=g) * 0.1
    return x, w, scale, bias


RECORDS = [(7, 3, 24), (7, 3, 6), (5, 3, 24)]   # K, n_f32, n_u8
SHAPES = [(16, 32), (18, 34)]


@pytest.mark.parametrize("Cout", [64, 128])
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("K,nf,nu", RECORDS)
def test_tail_walks_match_the_float64_convolution(eng, K, nf, nu, H, W, Cout):
    """dense walk (no flags) and dense + background walks chosen by flags derived from the data (image 0: renders in the top-left
    8x8 tile only, image 1: no renders at all), with and without the fused pool, against float64"""
    x, w, scale, bias = make_layer(K, nf, nu, H, W, Cout, seed=K * 1000 + nu * 10 + H + Cout)
    keep = torch.zeros(2, 1, H, W)
    keep[0, :, :8, :8] = 1.0
    x[:, nf:] *= keep
    st = Stem(eng, x, nf, K, w, scale, bias)
    assert st.forms == (3 if nu == 24 else 2)
    flags = tile_flags_of(x, nf)
    assert flags[0, 0, 0].item() == 1 and flags.sum().item() == 1
    pref = F.max_pool2d(st.ref, 3, 2, 1)
    for pool in (False, True):
        for fl in (None, flags):
            y, q = st.run(pool, fl)
            err = (st.nchw(y) - st.ref).abs().max().item()
            print(f"K{K} ({nf},{nu}) {H}x{W} Cout{Cout} pool={pool} flags={fl is not None}: err {err:.3e} / scale {st.scale:.3f}")
            assert err <= 2e-5 * st.scale, err
            full = y[: 2 * (st.Ho + 2) * (st.Wo + 2) * Cout].view(2, st.Ho + 2, st.Wo + 2, Cout)
            assert full[:, 0].abs().max() == 0 and full[:, -1].abs().max() == 0 and full[:, :, 0].abs().max() == 0 and full[:, :, -1].abs().max() == 0
            if pool:
                assert (st.pooled_nchw(q) - pref).abs().max().item() <= 2e-5 * st.scale


ONE_HOT = [
    # K, n_f32, n_u8, background walk, record slot, input channel of that slot
    (7, 3, 24, False, 32, 26),   # dense walk: the tail element = the last render channel
    (7, 3, 24, False, 0, 0),     # ... the first main element = first piece of the first crop channel
    (5, 3, 24, False, 32, 26),
    (5, 3, 24, False, 0, 0),
    (7, 3, 24, True, 8, 2),      # background walk: the tail element = third piece of the third crop channel
    (7, 3, 24, True, 0, 0),
    (7, 3, 6, True, 8, 2),       # the coarse record's background walk
    (7, 3, 6, True, 0, 0),
    (5, 3, 24, True, 8, 2),
    (5, 3, 24, True, 0, 0),
]


@pytest.mark.parametrize("K,nf,nu,background,slot,ch", ONE_HOT)
def test_one_hot_taps_reach_their_weights(eng, K, nf, nu, background, slot, ch):
    """the record is non-zero in ONE slot only (written directly: a lone third piece is no split of a channel value), and output channel
    ky * K + kx has ONE non-zero weight, at (ky, kx) of that slot's channel: every (ky, kx) at once, each output a single product"""
    N, H, W, Cout = 2, 18, 34, 64
    g = torch.Generator().manual_seed(K * 100 + slot + nu)
    integer = slot >= 3 * nf
    vals = torch.randint(1, 256, (N, H, W), generator=g).float()          # bf16-exact either way (8 significant bits)
    x = torch.zeros(N, nf + nu, H, W)
    x[:, ch] = vals / 255.0 if integer else vals / 64.0
    w = torch.zeros(Cout, nf + nu, K, K)
    for ky in range(K):
        for kx in range(K):
            w[ky * K + kx, ch, ky, kx] = 0.5 + torch.rand(1, generator=g).item()
    scale, bias = torch.ones(Cout), torch.zeros(Cout)
    pad = K // 2
    R = eng.xrec_elements(nf, nu)
    rec = eng.padded_nhwc(N, H, W, R, pad, "cuda", dtype=torch.bfloat16)
    eng.padded_view(rec, N, H, W, R, pad)[..., slot] = (vals if integer else vals / 64.0).cuda().to(torch.bfloat16)
    st = Stem(eng, x, nf, K, w, scale, bias, relu=False, rec=rec)
    flags = torch.zeros(N, (H + 7) // 8, (W + 7) // 8, dtype=torch.uint8, device="cuda") if background else None
    assert st.forms & (2 if background else 1)
    y, _ = st.run(False, flags)
    got = st.nchw(y)
    err = (got - st.ref).abs().max().item()
    print(f"K{K} ({nf},{nu}) background={background} slot {slot}: err {err:.3e} / scale {st.scale:.3f}")
    assert st.ref[:, : K * K].abs().amax(dim=(0, 2, 3)).min().item() > 0.1     # every (ky, kx) is exercised
    assert err <= 2e-5 * st.scale, err
    assert got[:, K * K :].abs().max().item() == 0


@pytest.mark.parametrize("Cout", [64, 128])
@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("K,nf,nu", RECORDS)
def test_background_walk_agrees_with_the_dense_walk(eng, K, nf, nu, H, W, Cout):
    """inputs whose render channels are all zero: any flags are valid.  All 0 (every workgroup on the background walk), all 1 (none),
    mixed per 8x8 tile (image 0: only the top-left tile set, so at 18 x 34 the last workgroup alone takes the background walk; image 1:
    a checkerboard)"""
    x, w, scale, bias = make_layer(K, nf, nu, H, W, Cout, seed=K * 1000 + nu * 10 + W + Cout + 1, renders=False)
    st = Stem(eng, x, nf, K, w, scale, bias)
    fy, fx = (H + 7) // 8, (W + 7) // 8
    zeros = torch.zeros(2, fy, fx, dtype=torch.uint8, device="cuda")
    mixed = zeros.clone()
    mixed[0, 0, 0] = 1
    mixed[1] = ((torch.arange(fy).view(-1, 1) + torch.arange(fx).view(1, -1)) % 2).to(torch.uint8).cuda()
    for pool in (False, True):
        y_dense, q_dense = st.run(pool, None)
        assert (st.nchw(y_dense) - st.ref).abs().max().item() <= 2e-5 * st.scale
        y_one, q_one = st.run(pool, torch.ones_like(zeros))
        assert torch.equal(y_one, y_dense) and (not pool or torch.equal(q_one, q_dense))   # SP launch, dense walk everywhere: same bits
        for name, fl in (("zeros", zeros), ("mixed", mixed)):
            if name == "zeros" and nu == 24:   # (counted for records of more than two chunks only)
                eng.profile_begin()
                eng.conv_stem_bg_stats(reset=True)
            y, q = st.run(pool, fl)
            if name == "zeros" and nu == 24:
                eng.profile_end()
                bg, total = eng.conv_stem_bg_stats(reset=True)
                assert total > 0 and bg == total, (bg, total)
            d = (y - y_dense).abs().max().item()
            print(f"K{K} ({nf},{nu}) {H}x{W} Cout{Cout} pool={pool} flags={name}: |background - dense| {d:.3e} / scale {st.scale:.3f}")
            assert d <= 2e-6 * st.scale, d
            if pool:
                assert (q - q_dense).abs().max().item() <= 2e-6 * st.scale


# ---- the switch ------------------------------------------------------------------------------------------------------------------------
SWITCH_MODELS = [("refiner", "vanilla_resnet34", 27, "pose", 9), ("coarse", "vanilla_resnet34", 9, "logits", 1)]


def switch_case(eng, name, kind, c_in, head, n_out):
    """(backbone, records, flags, b, h, w) of the switch test, everything from fixed seeds on the CPU"""
    from tests.support import synthetic as syn

    sd = syn.make_state_dict(kind, c_in, head, n_out, seed=11)
    bb = eng.Backbone(kind, c_in, head, n_out, sd)
    b, h, w = 2, 96, 128
    g = torch.Generator().manual_seed(c_in)
    x = torch.cat([torch.rand(b, 3, h, w, generator=g), torch.randint(0, 256, (b, c_in - 3, h, w), generator=g).float() / 255.0], dim=1)
    yy, xx = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    x[:, 3:] *= (((yy - 40) / 20.0) ** 2 + ((xx - 50) / 28.0) ** 2 < 1.0)      # renders inside an ellipse only
    assert bb.xrec_elements(3) == eng.xrec_elements(3, c_in - 3)
    return bb, to_records(eng, x, 3, bb.in_border), tile_flags_of(x, 3), b, h, w


def switch_outputs(eng, name, kind, c_in, head, n_out):
    bb, rec, flags, b, h, w = switch_case(eng, name, kind, c_in, head, n_out)
    res = {}
    for tag, fl in (("dense", 0), ("flags", flags.data_ptr())):
        out, feat = torch.empty(b, n_out, device="cuda"), torch.empty(b, 512, device="cuda")
        bb.forward(rec, b, h, w, out, None, feat, tile_flags=fl)
        torch.cuda.synchronize()
        res[f"{name}_{tag}_out"], res[f"{name}_{tag}_feat"] = out.cpu().numpy(), feat.cpu().numpy()
    return res


@pytest.mark.parametrize("model", SWITCH_MODELS, ids=[m[0] for m in SWITCH_MODELS])
def test_switch_off_reproduces_the_outputs_from_before_the_tail_plane(eng, model, monkeypatch):
    """MP_STEM_TAIL=0, read when the backbone is created: the stem keeps the walks without the tail plane, and a whole forward (without
    and with the rasteriser-style flags) gives the bits recorded on the same seeded inputs at the commit before the tail plane
    (switch_outputs there; tests/golden/stem_tail_switch_parent.npz).  The default agrees with them to fp32 round-off."""
    golden = np.load(GOLDEN)
    monkeypatch.setenv("MP_STEM_TAIL", "0")
    off = switch_outputs(eng, *model)
    for key, val in off.items():
        assert np.abs(golden[key]).max() > 0
        assert np.array_equal(val.view(np.uint32), golden[key].view(np.uint32)), key
    monkeypatch.delenv("MP_STEM_TAIL")
    on = switch_outputs(eng, *model)
    for key, val in on.items():
        fs = max(1.0, float(np.abs(golden[f"{model[0]}_{key.split('_')[1]}_feat"]).max()))
        assert np.abs(val - golden[key]).max() <= 1e-5 * fs, key
