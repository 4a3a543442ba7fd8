"""CPU: `megapose6d_amd.evaluation.bop_recall` (BOP 2019 average recalls, host arithmetic) on hand-made tables with known answers, and
the argument checks of the VSD front end that need no device."""
import numpy as np
import pandas as pd
import pytest

from megapose6d_amd import evaluation as ev

TAUS = [0.05 * k for k in range(1, 11)]
VSD_COLS = [f"vsd_{t:.2f}" for t in TAUS]


def table(vsd, mssd, mspd, diameter):
    n = len(mssd)
    d = {c: np.broadcast_to(np.asarray(vsd, np.float64), (n, 10))[:, k] for k, c in enumerate(VSD_COLS)}
    d.update(mssd=np.asarray(mssd, np.float64), mspd=np.asarray(mspd, np.float64), sym_id_mssd=np.zeros(n, np.int64), sym_id_mspd=np.zeros(n, np.int64),
             diameter=np.asarray(diameter, np.float64))
    return pd.DataFrame(d)


def test_column_names_are_the_ones_bop_errors_writes():
    assert ev._vsd_names(ev.BOP_TAUS) == VSD_COLS


def test_all_hits_and_all_misses():
    hit = ev.bop_recall(table(0.0, [0.0, 0.0], [0.0, 0.0], [0.1, 0.2]))
    assert hit == {"ar_vsd": 1.0, "ar_mssd": 1.0, "ar_mspd": 1.0, "ar": 1.0}
    miss = ev.bop_recall(table(1.0, [1.0, 1.0], [500.0, 500.0], [0.1, 0.2]))
    assert miss == {"ar_vsd": 0.0, "ar_mssd": 0.0, "ar_mspd": 0.0, "ar": 0.0}


def test_partial_recalls_count_threshold_by_threshold():
    # vsd error 0.22 everywhere: below theta = 0.25 ... 0.50 (6 of 10); mssd = 0.031 at diameter 0.1: below 0.035 ... 0.05 -> theta 0.35..0.50
    # (4 of 10); mspd 12 px: below 15 ... 50 (8 of 10)
    r = ev.bop_recall(table(0.22, [0.031], [12.0], [0.1]))
    assert r["ar_vsd"] == pytest.approx(0.6) and r["ar_mssd"] == pytest.approx(0.4) and r["ar_mspd"] == pytest.approx(0.8)
    assert r["ar"] == pytest.approx((0.6 + 0.4 + 0.8) / 3)
    # per-tau errors differ: a step from 1 to 0 after the third tau -> 7 of 10 taus are below every theta
    vsd = np.array([[1.0, 1.0, 1.0] + [0.0] * 7])
    assert ev.bop_recall(table(vsd, [0.0], [0.0], [0.1]))["ar_vsd"] == pytest.approx(0.7)


def test_nan_rows_are_misses():
    vsd = np.array([[0.0] * 10, [np.nan] * 10])
    r = ev.bop_recall(table(vsd, [0.0, np.nan], [0.0, np.nan], [0.1, 0.1]))
    assert r == {"ar_vsd": 0.5, "ar_mssd": 0.5, "ar_mspd": 0.5, "ar": 0.5}


def test_image_width_scales_the_pixel_thresholds():
    t = table(0.0, [0.0], [12.0], [0.1])
    assert ev.bop_recall(t, image_width=640)["ar_mspd"] == pytest.approx(0.8)       # thresholds 5 ... 50
    assert ev.bop_recall(t, image_width=1280)["ar_mspd"] == pytest.approx(0.9)      # 10 ... 100: only 10 is not above 12
    assert ev.bop_recall(t, image_width=320)["ar_mspd"] == pytest.approx(0.6)       # 2.5 ... 25: 12.5, 15, ..., 25


def test_the_comparison_is_strict():
    # an error exactly on a threshold is a miss at that threshold: mspd = 10 px misses theta = 5 and 10; mssd = 0.5 * diameter misses all
    r = ev.bop_recall(table(0.5, [0.25], [10.0], [0.5]))
    assert r["ar_mspd"] == pytest.approx(0.8) and r["ar_mssd"] == 0.0 and r["ar_vsd"] == 0.0
    r = ev.bop_recall(table(np.nextafter(0.5, 0), [np.nextafter(0.25, 0)], [np.nextafter(10.0, 0)], [0.5]))
    assert r["ar_mspd"] == pytest.approx(0.9) and r["ar_mssd"] == pytest.approx(0.1) and r["ar_vsd"] == pytest.approx(0.1)


def test_unbuilt_modes_raise_value_error():
    import torch

    z = torch.zeros(1, 4, 4)
    K = torch.eye(3)[None]
    with pytest.raises(ValueError):
        ev.vsd(z, z, z, K, torch.ones(1), cost_type="tlinear")
    with pytest.raises(ValueError):
        ev.vsd(z, z, z, K, torch.ones(1), visib_mode="bop18")
    with pytest.raises(ValueError):
        ev.bop_recall(pd.DataFrame(dict(mssd=[0.0], mspd=[0.0], diameter=[0.1])))
