"""CPU: the stage-by-stage backbone references (tests/support/backbone_ref.py) against the end-to-end restatement they are cut from
(oracle/backbones.py): composed in float32 they ARE net_forward, bit for bit; in float64 they agree with it to float32 round-off; and the
shifted-matmul convolution the GPU tests use on the device equals F.conv2d in float64."""
import pytest
import torch
import torch.nn.functional as F

from oracle import backbones as ob
from tests.support import synthetic as syn
from tests.support.backbone_ref import BackboneRef, conv_matmul

CASES = [("vanilla_resnet34", 9, "logits", 1), ("resnet34", 32, "pose", 9), ("resnet18", 9, "logits", 1), ("resnet34_width=2", 9, "logits", 1)]
H, W, B = 50, 70, 2   # odd maps at every level: 25x35, 13x18, 7x9, 4x5, 2x3


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"{c[0]}-{c[1]}")
def net(request):
    kind, c_in, head, n_out = request.param
    sd = syn.make_state_dict(kind, c_in, head, n_out, seed=2)
    x = torch.rand(B, c_in, H, W, generator=torch.Generator().manual_seed(7))
    with torch.no_grad():
        return kind, sd, x, ob.net_forward(sd, kind, x)


def test_stages_composed_in_float32_are_the_oracle(net):
    kind, sd, x, want = net
    ref = BackboneRef(sd, kind, dtype=torch.float32)
    with torch.no_grad():
        got = ref.forward(x)
    assert set(got) == set(want)
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_stages_in_float64_agree_to_float32_round_off(net):
    """~36 convolutions deep, each adding about 1e-6 of its scale in float32: 1e-4 of the output scale bounds the oracle's own error"""
    kind, sd, x, want = net
    ref = BackboneRef(sd, kind, dtype=torch.float64)
    with torch.no_grad():
        got = ref.forward(x.double())
    for k in want:
        err = (got[k] - want[k].double()).abs().max().item()
        assert err < 1e-4 * max(1.0, got[k].abs().max().item()), (k, err)


def test_stage_pieces_are_the_ones_the_blocks_use(net):
    """downsample() and next_act(), which the GPU tests compare on their own, are what stage() applies inside: rebuilding block 0 of
    stage 2 from them gives stage 2's first block"""
    kind, sd, x, _ = net
    ref = BackboneRef(sd, kind, dtype=torch.float64)
    with torch.no_grad():
        l1 = ref.stage(1, ref.stem(x.double()))
        P = "backbone.layer2.0."
        if ref.wide:
            a = ref.next_act(1, l1)
            out = F.relu(ref._bn(P + "bn2", F.conv2d(a, ref.sd[P + "conv1.weight"], stride=2, padding=1)))
            want = F.conv2d(out, ref.sd[P + "conv2.weight"], padding=1) + ref.downsample(2, a)
        else:
            out = F.relu(ref._bn(P + "bn1", F.conv2d(l1, ref.sd[P + "conv1.weight"], stride=2, padding=1)))
            want = F.relu(ref._bn(P + "bn2", F.conv2d(out, ref.sd[P + "conv2.weight"], padding=1)) + ref.downsample(2, l1))
        assert torch.equal(ref.block(2, 0, l1), want)
        assert want.shape[-2:] == (7, 9)


@pytest.mark.parametrize("K,stride,pad", [(7, 2, 3), (5, 2, 2), (3, 1, 1), (3, 2, 1), (1, 2, 0)])
def test_shifted_matmul_convolution_equals_conv2d_in_float64(K, stride, pad):
    g = torch.Generator().manual_seed(K * 10 + stride)
    x = torch.randn(2, 12, 13, 18, generator=g, dtype=torch.float64)
    w = torch.randn(24, 12, K, K, generator=g, dtype=torch.float64)
    want = F.conv2d(x, w, stride=stride, padding=pad)
    got = conv_matmul(x, w, stride=stride, padding=pad)
    assert got.shape == want.shape
    assert (got - want).abs().max().item() < 1e-12 * want.abs().max().item()


def test_matmul_form_gives_the_same_network(net):
    kind, sd, x, _ = net
    with torch.no_grad():
        a = BackboneRef(sd, kind, dtype=torch.float64).forward(x.double())
        b = BackboneRef(sd, kind, dtype=torch.float64, conv=conv_matmul).forward(x.double())
    for k in a:
        assert (a[k] - b[k]).abs().max().item() < 1e-11 * max(1.0, a[k].abs().max().item()), k
