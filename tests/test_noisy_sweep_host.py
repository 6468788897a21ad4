"""CPU: the host twin of the noisy moving-sensor sweeps (lrc_noisy_sweep_rays, compiled from the kernel's own
gen_ray_noisy_sweep) against the numpy restatement (tests/noisy_sweep_restate.py: the composition of the noise and the sweep
restatements), bit for bit; the identities that tie it to the two generators it joins; the draw conditions of the inputs the
GPU tests use; the argument checks."""
import numpy as np
import pytest

import noise_restate as nr
from helpers import assert_bit_equal
from noisy_sweep_restate import noisy_sweep_rays
from sweep_restate import sweep_rays
from test_noise_gpu import _table
from test_sweep_gpu import MOTIONS, _sweeps

SEED = 0xC0FFEE123456789
P = 3


@pytest.fixture(scope="module")
def tab():
    from lidarcast import noise
    return noise.table()


def _fire(width, lines=4):
    return (np.arange(lines * width) % width) / width


def _records(motion, n=P):
    from lidarcast import motion_records
    starts, ends = _sweeps("synth_A1_office", n, *MOTIONS[motion])
    return motion_records(starts, ends), starts


def _model(first=0, **kw):
    from lidarcast.noise import NoiseModel
    par = dict(range_std=0.02, angle_std=0.01, dropout=0.05)
    par.update(kw)
    return NoiseModel(seed=SEED, first_frame=first, **par)


def _assert_twin(got, rays, cen, term, keep, what):
    assert_bit_equal(got["rays"], rays, f"{what}: rays")
    assert_bit_equal(got["centres"], cen, f"{what}: centres")
    assert_bit_equal(got["range_term"], term, f"{what}: range term")
    assert np.array_equal(got["keep"], keep), f"{what}: keep"


@pytest.mark.parametrize("first", [0, 2 ** 32 - 1])
@pytest.mark.parametrize("motion", list(MOTIONS))
@pytest.mark.parametrize("width", [100, 96])
def test_host_twin_is_the_restatement(tab, width, motion, first):
    from lidarcast import noise
    dirs, fire = _table(4, width), _fire(width)
    rec, _ = _records(motion)
    assert np.allclose(2 * np.arccos(rec[:, 12]), 0.1 if motion == "realistic" else 0.4, atol=1e-3)
    m = _model(first)
    rays, cen, term, keep, rows = noisy_sweep_rays(rec, dirs, fire, m, *tab)
    got = noise.sweep_rays(m, rec, dirs, fire)
    _assert_twin(got, rays, cen, term, keep, f"4x{width} {motion} first {first}")
    # the inputs exercise what they are for
    N = len(dirs)
    assert 0 < (~keep).sum() < 0.2 * P * N                                    # dropout 0.05 over 1200 (1152) rays
    flat = rows.reshape(-1, 3)
    assert (flat != np.tile(dirs, (P, 1))).any(axis=1).mean() > 0.95          # the rows are jittered ...
    assert_bit_equal(flat[7::N], np.tile(dirs[7], (P, 1)))                    # ... but for the two with h == 0
    assert_bit_equal(flat[11::N], np.tile(dirs[11], (P, 1)))
    clean, _ = sweep_rays(rec, dirs, fire)
    for r in (7, 11):                                                         # the twin leaves them alone as well
        sel = np.arange(P) * N + r
        sel = sel[keep[sel]]
        assert_bit_equal(got["rays"][sel], clean[sel])
    assert (got["rays"][keep][:, 3:] != clean[keep][:, 3:]).any(axis=1).mean() > 0.95
    assert term.any() and np.isnan(got["rays"][~keep][:, 3:]).all() and np.isfinite(got["rays"][keep]).all()


@pytest.mark.parametrize("width", [100, 96])
def test_all_zero_model_is_the_sweep(width):
    from lidarcast import noise
    from lidarcast.noise import NoiseModel
    dirs, fire = _table(4, width), _fire(width)
    for motion in MOTIONS:
        rec, _ = _records(motion)
        rays, cen = sweep_rays(rec, dirs, fire)
        got = noise.sweep_rays(NoiseModel(seed=99, first_frame=17), rec, dirs, fire)
        _assert_twin(got, rays, cen, np.zeros(len(rays), np.float32), np.ones(len(rays), bool), f"zero model {motion}")


@pytest.mark.parametrize("first", [0, 2 ** 32 - 1])
@pytest.mark.parametrize("width", [100, 96])
def test_static_sweeps_are_the_static_noisy_scan(tab, width, first):
    """end == start, and separately a zero fire table: the rays of noise_restate.noisy_rays under the start poses.  dgemm_row
    never yields -0.0, so the sweep adds signed zeros only."""
    from lidarcast import motion_records, noise
    dirs, fire = _table(4, width), _fire(width)
    N = len(dirs)
    m = _model(first)
    for motion in MOTIONS:
        rec, starts = _records(motion)
        rays, cen, term, keep, _ = nr.noisy_rays(starts, dirs, m.seed, m.first_frame, m.range_std, m.angle_std, m.dropout, *tab)
        cen = np.repeat(cen, N, axis=0)
        for what, r, f in (("end == start", motion_records(starts, starts), fire), ("zero fire table", rec, np.zeros(N))):
            _assert_twin(noise.sweep_rays(m, r, dirs, f), rays, cen, term, keep, f"{what} {motion}")


def test_frames_do_not_depend_on_the_call():
    from lidarcast import noise
    dirs, fire = _table(4, 100), _fire(100)
    rec, _ = _records("extreme", 6)
    m = _model(2 ** 32 - 3)
    whole = noise.sweep_rays(m, rec, dirs, fire)
    a = noise.sweep_rays(m, rec[:2], dirs, fire)
    b = noise.sweep_rays(m.at_frame(m.first_frame + 2), rec[2:], dirs, fire)
    for k in ("rays", "centres", "range_term"):
        assert_bit_equal(whole[k], np.concatenate([a[k], b[k]]), k)
    assert np.array_equal(whole["keep"], np.concatenate([a["keep"], b["keep"]]))
    other = noise.sweep_rays(m.at_frame(0), rec, dirs, fire)
    assert (other["range_term"] != whole["range_term"]).mean() > 0.95


def test_arguments_are_checked():
    from lidarcast import noise
    from lidarcast.noise import NoiseModel
    dirs, fire = _table(4, 96), _fire(96)
    rec, _ = _records("realistic")
    for bad in (dict(range_std=-1.0), dict(range_std=float("nan")), dict(range_std=float("inf")), dict(angle_std=float("inf")),
                dict(angle_std=-0.1), dict(angle_std=float("nan")), dict(dropout=1.0), dict(dropout=-0.5),
                dict(dropout=float("nan"))):
        with pytest.raises(ValueError, match="lrc_noisy_sweep_rays"):
            noise.sweep_rays(NoiseModel(seed=1, **bad), rec, dirs, fire)
        with pytest.raises(ValueError, match="lrc_noisy_sweep_rays"):       # an empty call checks the model too
            noise.sweep_rays(NoiseModel(seed=1, **bad), rec[:0], dirs, fire)
    m = NoiseModel(seed=1, range_std=0.01)
    for v in (1.0, -0.1, np.nan):
        with pytest.raises(ValueError, match=r"fire\[3\]"):
            noise.sweep_rays(m, rec, dirs, np.where(np.arange(len(fire)) == 3, v, fire))
    with pytest.raises(ValueError):
        noise.sweep_rays(m, rec, dirs, fire[:-1])
    for j, v, why in ((12, 0.7, "pi/2"), (13, 0.5, "non-unit"), (5, np.inf, "not finite"), (17, np.nan, "not finite")):
        r = rec.copy()
        r[1, j] = v
        with pytest.raises(ValueError, match=why):
            noise.sweep_rays(m, r, dirs, fire)
    assert noise.sweep_rays(m, rec[:0], dirs, fire)["rays"].shape == (0, 6)
