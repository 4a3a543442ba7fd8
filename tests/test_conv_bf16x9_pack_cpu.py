"""CPU tier: the host-side weight packs of the exact-piece convolutions (mp_conv_bf16x9_pack_weights, csrc/conv_bf16x9.hip;
mp_conv_wino_bf16_pack_weights, csrc/conv_wino_bf16.hip).

The three bf16 pieces of every packed weight add back, bit for bit, to the fp32 weight the fp32 kernel's pack holds (w * scale, one
fp32 multiplication), in MFMA fragment order [n block][K slice][32-column block][piece][lane][8]; every padded slot is zero.  The same
holds for the Winograd pair: the pieces add back to the U = G g G^T the fp32 Winograd pack holds (one transform feeds both packs).
The packs run in a child process: this file sorts first in the CPU tier, and loading the engine library (and the HIP runtime behind
it) there would change what the suite's own process has loaded before the CPU oracle tests that follow.
"""
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]

_PACK = """
import sys
import numpy as np
from megapose6d_amd import engine
a = np.load(sys.argv[1])
np.save(sys.argv[2], engine.conv_bf16x9_pack_weights(a["w"], int(a["cin_p"]), a["scale"]))
"""

_PACK_WINO = """
import sys
import numpy as np
from megapose6d_amd import engine
a = np.load(sys.argv[1])
np.save(sys.argv[2], engine.conv_wino_pack_weights(a["w"], int(a["cin_p"]), a["scale"]))
np.save(sys.argv[3], engine.conv_wino_bf16_pack_weights(a["w"], int(a["cin_p"]), a["scale"]))
"""


def _pieces_as_f32(blob_u16):
    return (blob_u16.astype(np.uint32) << 16).view(np.float32)


@pytest.mark.parametrize("Cout,Cin,K,cin_p", [(128, 64, 3, 64), (256, 128, 1, 128), (192, 40, 3, 48), (64, 16, 1, 32)])
def test_bf16x9_pack_adds_back_to_the_fp32_weights(tmp_path, Cout, Cin, K, cin_p):
    rng = np.random.default_rng(Cout + Cin + K)
    w = (rng.standard_normal((Cout, Cin, K, K)) * np.exp(rng.uniform(-30, 30, (Cout, Cin, K, K)))).astype(np.float32)
    scale = (rng.random(Cout) + 0.5).astype(np.float32)
    np.savez(tmp_path / "in.npz", w=w, scale=scale, cin_p=cin_p)
    subprocess.run([sys.executable, "-c", _PACK, str(tmp_path / "in.npz"), str(tmp_path / "blob.npy")], cwd=ROOT, check=True, timeout=300)
    blob = np.load(tmp_path / "blob.npy").view(np.uint16)
    n_blk = (Cout + 127) // 128
    k_total = K * K * cin_p
    n_sl = 2 * ((k_total + 31) // 32)
    assert blob.size == n_blk * n_sl * 4 * 3 * 64 * 8
    p = _pieces_as_f32(blob).reshape(n_blk, n_sl, 4, 3, 64, 8)
    # back to [n][k]: n = 128 nb + 32 j + (lane & 31), k = 16 t + 8 (lane >> 5) + e
    p = p.reshape(n_blk, n_sl, 4, 3, 2, 32, 8).transpose(3, 0, 2, 5, 1, 4, 6).reshape(3, n_blk * 128, n_sl * 16)
    total = (p[0] + p[1]) + p[2]   # exact in fp32: the pieces partition the significand
    want = np.zeros((n_blk * 128, n_sl * 16), dtype=np.float32)
    wk = np.zeros((Cout, K, K, cin_p), dtype=np.float32)
    wk[..., :Cin] = (w * scale[:, None, None, None]).transpose(0, 2, 3, 1)   # k = kh * (KW * Cin_p) + kw * Cin_p + c
    want[:Cout, :k_total] = wk.reshape(Cout, k_total)
    assert np.array_equal(total.view(np.uint32), want.view(np.uint32))
    # every piece is a bf16 value, ordered by magnitude (truncation keeps the sign of every piece)
    assert np.all(np.abs(p[1]) <= np.abs(p[0])) and np.all(np.abs(p[2]) <= np.abs(p[1]))


@pytest.mark.parametrize("Cout,Cin,cin_p", [(64, 16, 16), (128, 40, 48)])
def test_wino_packs_hold_the_same_transformed_weights(tmp_path, Cout, Cin, cin_p):
    """mp_conv_wino_pack_weights and mp_conv_wino_bf16_pack_weights store the same U[f] per (cout, cin): the three pieces of the
    bf16 blob add back, bit for bit, to the fp32 blob's value; padded input channels are zero in both."""
    rng = np.random.default_rng(Cout + Cin)
    w = (rng.standard_normal((Cout, Cin, 3, 3)) * np.exp(rng.uniform(-30, 30, (Cout, Cin, 3, 3)))).astype(np.float32)
    scale = (rng.random(Cout) + 0.5).astype(np.float32)
    np.savez(tmp_path / "in.npz", w=w, scale=scale, cin_p=cin_p)
    subprocess.run([sys.executable, "-c", _PACK_WINO, str(tmp_path / "in.npz"), str(tmp_path / "u.npy"), str(tmp_path / "ub.npy")], cwd=ROOT,
                   check=True, timeout=300)
    n_cb = Cout // 64
    # fp32 blob [cb][chunk][f][j][lane][q]: cin = 8 chunk + 4 (lane >> 5) + q, cout = 64 cb + 32 j + (lane & 31)
    u = np.load(tmp_path / "u.npy")
    assert u.dtype == np.float32 and u.size == 16 * cin_p * Cout
    u = u.reshape(n_cb, cin_p // 8, 16, 2, 2, 32, 4).transpose(0, 3, 5, 1, 4, 6, 2).reshape(Cout, cin_p, 16)
    # piece blob [cb][step][f][j][piece][lane][e]: cin = 16 step + 8 (lane >> 5) + e
    ub = np.load(tmp_path / "ub.npy").view(np.uint16)
    assert ub.size == 3 * 16 * cin_p * Cout
    p = _pieces_as_f32(ub).reshape(n_cb, cin_p // 16, 16, 2, 3, 2, 32, 8).transpose(4, 0, 3, 6, 1, 5, 7, 2).reshape(3, Cout, cin_p, 16)
    total = (p[0] + p[1]) + p[2]   # exact in fp32: the pieces partition the significand
    assert np.array_equal(total.view(np.uint32), u.view(np.uint32))
    assert np.count_nonzero(u[:, :Cin]) > 0.99 * Cout * Cin * 16   # (the unpacking above looks at the real channels)
    assert not u[:, Cin:].view(np.uint32).any() and not p[:, :, Cin:].view(np.uint32).any()
    assert np.all(np.abs(p[1]) <= np.abs(p[0])) and np.all(np.abs(p[2]) <= np.abs(p[1]))
