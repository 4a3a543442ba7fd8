"""CPU tier: the host-side weight pack of the exact-piece direct convolution (mp_conv_bf16x9_pack_weights, csrc/conv_bf16x9.hip).

The three bf16 pieces of every packed weight add back, bit for bit, to the fp32 weight the fp32 kernel's pack holds (w * scale, one
fp32 multiplication), in MFMA fragment order [n block][K slice][32-column block][piece][lane][8]; every padded slot is zero.
The pack runs in a child process: this file sorts first in the CPU tier, and loading the engine library (and the HIP runtime behind
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
