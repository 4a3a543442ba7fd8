"""The piece blobs of the stem's tail-plane walks (csrc/conv_stem.hip, mp_conv_stem_pack_weights_tail), unpacked on the host.

A tail walk visits, per tap, only the record chunks in front of the lone last real element (the "main" slices, in the present
(ky, kx, chunk) order), then one tail slice per kernel row whose element e < K is the tail element's weight at (ky, kx = e), then zero
padding up to an even number of steps of 4 slices.  Checked for the dense walk (33 real elements: 7x7 62 -> 52 steps) and the background
walk (the 9 crop pieces: 26 -> 14 steps, also for the coarse net's 16-element record):
  * every (ky, kx, element, piece) weight of the real elements appears exactly once, at the place the walk reads it;
  * every other position of the blob (element padding, slice padding) is zero;
  * the three pieces of each weight are, bit for bit, the pieces the present packer (mp_conv_stem_pack_weights_mask) produces, and sum
    exactly to its fp32 weight.
"""
import numpy as np
import pytest


def steps_of(slices: int) -> int:
    return ((slices + 3) // 4 + 1) // 2 * 2


def unpack(blob: np.ndarray, Cout: int, T: int) -> np.ndarray:
    """uint8 blob [cb][wave][step][piece][lane][8 bf16] -> float32 [Cout][slice = 4 step + (lane >> 4)][piece][8] (bf16 -> fp32 is exact)"""
    u = blob.view(np.uint16).reshape(Cout // 64, 4, T, 3, 4, 16, 8)            # lane = group * 16 + (cout & 15)
    f = (u.astype(np.uint32) << 16).view(np.float32)
    return f.transpose(0, 1, 5, 2, 4, 3, 6).reshape(Cout, 4 * T, 3, 8)         # [cb, wave, i][step, group][piece][e]


CASES = [
    # K, n_f32, n_u8, background, steps
    (7, 3, 24, False, 52),
    (7, 3, 24, True, 14),
    (7, 3, 6, True, 14),      # the coarse record: no tail in its dense walk (15 real elements), one in the background walk
    (5, 3, 24, False, 28),
    (5, 3, 24, True, 8),
    (7, 4, 21, False, 52),    # 12 + 21 = 33 real elements with four fp32-kind channels
]


@pytest.mark.parametrize("K,nf,nu,background,steps", CASES)
def test_tail_blob_holds_every_real_weight_once_and_zeros_elsewhere(K, nf, nu, background, steps):
    from megapose6d_amd import engine as eng

    Cout, Cin = 128, nf + nu
    rng = np.random.RandomState(K * 100 + nf * 10 + nu + int(background))
    w = rng.standard_normal((Cout, Cin, K, K)).astype(np.float32)
    scale = (rng.rand(Cout) + 0.5).astype(np.float32)
    n_real = 3 * nf if background else 3 * nf + nu          # the elements this walk needs
    assert n_real % 8 == 1 and eng.conv_stem_tail_forms(K, nf, nu) & (2 if background else 1)
    qm = n_real // 8                                          # main chunks per pixel
    S_main, S = K * K * qm, K * K * qm + K
    T = steps_of(S)
    assert T == steps
    blob = eng.conv_stem_pack_weights_tail(w, nf, scale, background=background)
    assert blob is not None and blob.size == (Cout // 64) * 4 * T * 3072
    got = unpack(blob, Cout, T)

    # the present packer's pieces of the same weights, by (cout, ky, kx, record slot): its dense walk is slice = (ky * K + kx) * Q + q
    Q = eng.xrec_elements(nf, nu) // 8
    Td = steps_of(K * K * Q)
    dense = unpack(eng.conv_stem_pack_weights(w, nf, scale), Cout, Td)[:, : K * K * Q].reshape(Cout, K, K, Q, 3, 8)
    ref = dense.transpose(0, 1, 2, 4, 3, 5).reshape(Cout, K, K, 3, Q * 8)     # [cout][ky][kx][piece][slot]
    # ... which sum exactly to fl32(w * scale [/ 255]) (exact truncation split: (p1 + p2) + p3 == the weight)
    f = np.where(np.arange(Q * 8) < 3 * nf, 1.0, 1.0 / 255.0)
    ch = np.array([s // 3 if s < 3 * nf else nf + (s - 3 * nf) for s in range(3 * nf + nu)])
    wref = (w.astype(np.float64) * scale.astype(np.float64)[:, None, None, None])[:, ch].transpose(0, 2, 3, 1) * f[: 3 * nf + nu]
    wref = wref.astype(np.float32)                                             # [cout][ky][kx][slot]
    assert np.array_equal((ref[:, :, :, 0] + ref[:, :, :, 1]) + ref[:, :, :, 2], np.concatenate(
        [wref, np.zeros((Cout, K, K, Q * 8 - wref.shape[-1]), np.float32)], axis=-1))

    count = np.zeros((K, K, n_real), dtype=np.int64)
    expect = np.zeros_like(got)
    for s in range(S):
        if s < S_main:
            ky, r = divmod(s, K * qm)
            kx, q = divmod(r, qm)
            for e in range(8):
                count[ky, kx, 8 * q + e] += 1
                expect[:, s, :, e] = ref[:, ky, kx, :, 8 * q + e]
        else:
            ky = s - S_main
            for e in range(K):
                count[ky, e, 8 * qm] += 1
                expect[:, s, :, e] = ref[:, ky, e, :, 8 * qm]
    assert (count == 1).all()                                   # every (ky, kx, real element) is walked exactly once ...
    assert np.array_equal(got.view(np.uint32), expect.view(np.uint32))   # ... with the present packer's three pieces; all else is zero
    assert not got[:, S:].any() and not got[:, S_main:S, :, K:].any()    # (padding slices; elements K .. 7 of the tail slices)
    # the three pieces of each walked weight sum exactly to the present packer's fp32 weight
    tail = got[:, S_main:S, :, :K]                                        # [cout][ky][piece][kx]
    assert np.array_equal((tail[:, :, 0] + tail[:, :, 1]) + tail[:, :, 2], wref[:, :, :, 8 * qm])
    assert np.abs(wref[:, :, :, :n_real]).min() > 0                       # (no accidental zeros among the real weights)


def test_records_without_a_lone_tail_element_have_no_tail_form():
    from megapose6d_amd import engine as eng

    assert eng.conv_stem_tail_forms(7, 3, 24) == 3 and eng.conv_stem_tail_forms(5, 3, 24) == 3
    assert eng.conv_stem_tail_forms(7, 3, 6) == 2                # coarse: 15 real elements, 9 crop pieces
    assert eng.conv_stem_tail_forms(7, 8, 24) == 0               # RGBD, Q = 6: 48 real elements
    assert eng.conv_stem_tail_forms(7, 4, 28) == 0               # 40 real elements; 12 fp32-kind pieces
    assert eng.conv_stem_tail_forms(7, 5, 26) == 0               # 41 real elements, but the widened 7x7 / Q = 6 patch does not fit
    assert eng.conv_stem_tail_forms(5, 5, 26) == 1               # ... the 5x5 one does
    w = np.zeros((64, 32, 7, 7), np.float32)
    assert eng.conv_stem_pack_weights_tail(w, 8) is None and eng.conv_stem_pack_weights_tail(w, 8, background=True) is None
