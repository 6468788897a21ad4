"""CPU tests of tests/full_parity.py: the whole-trajectory statement equals the oracle called pose by pose (and brute force
on a slice), and the comparator sees each kind of defect -- one planted defect per test, so that a comparator which ignores
a field cannot pass -- and says where it sits (pose, tile, lane)."""
import re

import numpy as np
import pytest

import full_parity as fp
from helpers import assert_bit_equal, pose, sensor_small
from sweep_restate import sweep_rays

P, LINES, WIDTH = 5, 4, 96            # N = 384: six tiles per pose
N = LINES * WIDTH


def _rot(yaw, pitch, roll):
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    Rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1]])
    Ry = np.array([[cp, 0, sp], [0, 1, 0], [-sp, 0, cp]])
    Rx = np.array([[1, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return Rz @ Ry @ Rx


@pytest.fixture(scope="module")
def room():
    from lidarcast import synth
    from oracle.c_oracle import OracleMesh
    mesh = synth.make_room(size=(4, 3, 2.5), num_boxes=4, seed=5, cell=0.05)
    return mesh, OracleMesh(mesh.vertices, mesh.triangles).build()


def _poses():
    poses = np.stack([pose(0.8 + 0.6 * i, 1.2 + 0.1 * i, 0.9 + 0.1 * i, yaw=0.5 * i) for i in range(P)])
    poses[3, :3, :3] = _rot(0.4, -0.7, 1.1)          # pitched and rolled
    poses[4, :3, 3] = (0.06, 1.5, 1.0)               # centimetres from a wall
    return poses


@pytest.fixture(scope="module")
def want(room):
    mesh, om = room
    w = fp.expected_sensor_scan(om, mesh, sensor_small(LINES, WIDTH, max_range=1.6), _poses(), threads=4)
    assert 0.2 < w["keep"].mean() < 0.9               # the strict filter decides a large share of the rays
    return w


def test_whole_trajectory_equals_the_oracle_pose_by_pose(room, want):
    from lidar import create_lidar
    from oracle import np_oracle
    mesh, om = room
    k = sensor_small(LINES, WIDTH, max_range=1.6)
    poses = _poses()
    assert (want["P"], want["N"]) == (P, N) and want["counts"].sum() == len(want["rows"]) == want["keep"].sum()
    got = list(fp.frames(want))
    for p in range(P):
        lidar = create_lidar(k, poses[p])
        pts, _, idx = np_oracle.lidar_intersect_mesh(om, lidar, threads=2, return_index=True)
        t, prim = om.cast(lidar.get_rays(), threads=2)
        sl = slice(p * N, (p + 1) * N)
        keep = want["keep"][sl]
        assert np.array_equal(np.flatnonzero(keep), idx) and want["counts"][p] == len(idx)
        assert_bit_equal(want["point3"][sl][keep], pts, f"pose {p} points")
        assert_bit_equal(want["t"][sl][keep], t[idx])
        assert_bit_equal(want["prim"][sl][keep], prim[idx])
        assert_bit_equal(want["normal3"][sl][keep], om.normals(prim[idx]))
        assert np.array_equal(want["sem"][sl][keep], mesh.triangle_sem[prim[idx]])
        assert np.array_equal(want["ins"][sl][keep], mesh.triangle_ins[prim[idx]])
        # removed rays are reported exactly like misses
        assert np.isposinf(want["t"][sl][~keep]).all() and (want["prim"][sl][~keep] == fp.MISS).all()
        for a in ("point3", "normal3", "sem", "ins"):
            assert not want[a][sl][~keep].any()
        gi, gp, gs, gn = got[p]
        assert np.array_equal(gi, idx)
        assert_bit_equal(gp, pts)
        assert np.array_equal(gs, mesh.triangle_sem[prim[idx]]) and np.array_equal(gn, mesh.triangle_ins[prim[idx]])
    lab = want["rows"][:, 3].copy().view(np.uint32)
    keep = want["keep"]
    assert np.array_equal(lab, want["sem"][keep].astype(np.uint32) | (want["ins"][keep].astype(np.uint32) << 16))
    assert (want["ins"] != 0).any() and (want["sem"] != 0).any()       # the label packing is exercised in both halves


def test_unfiltered_scan_equals_brute_force_on_a_slice(room):
    mesh, om = room
    rays, cen = fp.sensor_rays(sensor_small(LINES, WIDTH), _poses())
    w = fp.expected_scan(om, rays, cen, np.inf, P, mesh.triangle_sem, mesh.triangle_ins, threads=3)
    sl = slice(N + 100, 3 * N - 50)
    t, prim = om.brute(rays[sl])
    assert_bit_equal(w["t"][sl], t)
    assert_bit_equal(w["prim"][sl], prim)
    assert np.isfinite(t).mean() > 0.99


def test_one_centre_per_ray_equals_the_oracle_column_by_column(room):
    """Moving-sensor sweeps: every column has its own range-filter centre (sweep_restate.sweep_rays)."""
    from lidar import IndoorLidar
    from lidarcast import motion_records
    from oracle import np_oracle
    mesh, om = room
    k = sensor_small(4, 32, max_range=1.4)
    lid = IndoorLidar(k, np.eye(4))
    dirs, fire = lid.sensor_directions(), lid.firing_fractions()
    starts = np.stack([pose(1.0, 1.2, 1.0, yaw=0.2), pose(2.5, 1.6, 1.2, yaw=-1.0)])
    ends = np.stack([pose(1.3, 1.3, 1.0, yaw=0.5), pose(2.4, 1.9, 1.2, yaw=-0.7)])
    rays, cen = sweep_rays(motion_records(starts, ends), dirs, fire)
    n = len(dirs)
    w = fp.expected_scan(om, rays, cen, k.max_range, 2, mesh.triangle_sem, mesh.triangle_ins, threads=2)
    assert 0.1 < w["keep"].mean() < 0.95
    for s in range(2):
        for col in range(32):
            sel = s * n + np.arange(4) * 32 + col
            assert (cen[sel] == cen[sel[0]]).all()

            class Column:
                intrinsics = k
                pose = pose(*cen[sel[0]])
                def get_rays(self):
                    return rays[sel]
            pts, _, idx = np_oracle.lidar_intersect_mesh(om, Column(), return_index=True)
            assert np.array_equal(np.flatnonzero(w["keep"][sel]), idx)
            assert_bit_equal(w["point3"][sel][idx], pts)


# ---- discrimination: one planted defect each ------------------------------------------------------------------------------
def _copy(want, fill=-7.0, spare=10):
    got = {f: want[f].copy() for f in fp.RECORDS + ("counts",)}
    got["rows"] = np.concatenate([want["rows"], np.full((spare, 4), fill, np.float32)])
    got["fill"] = fill
    return got


def _kept_ray(want, p, after):
    """A kept ray of pose p at or after in-pose index `after`, as a flat index."""
    k = np.flatnonzero(want["keep"][p * N:(p + 1) * N])
    return p * N + int(k[k >= after][0])


def _expect_failure(got, want, pattern):
    with pytest.raises(AssertionError) as e:
        fp.assert_scan_equal(got, want, "planted")
    assert re.search(pattern, str(e.value)), str(e.value)
    return str(e.value)


def test_an_exact_copy_passes(want):
    assert fp.assert_scan_equal(_copy(want), want, "copy") == P * N
    assert fp.differences(_copy(want), want, fp.RECORDS + fp.CLOUD) == (0, [])
    shaped = _copy(want)
    for f in fp.RECORDS:                                # (P, N, ...) records are accepted as they are
        shaped[f] = shaped[f].reshape((P, N) + shaped[f].shape[1:])
    fp.assert_scan_equal(shaped, want, "shaped")
    exact = _copy(want, spare=0)                        # exactly K rows: nothing beyond them to check
    del exact["fill"]
    fp.assert_scan_equal(exact, want, "exact")


def test_t_off_by_one_bit_is_seen_and_located(want):
    i = _kept_ray(want, 2, 200)
    got = _copy(want)
    got["t"].view(np.uint32)[i] ^= 1
    msg = _expect_failure(got, want, r"^planted: 1 of 1920 rays differ\n  t: 1 of 1920 rays differ")
    r = i % N
    assert f"pose 2, tile {r // 64} of the pose (tile {i // 64} of the scan), lane {r % 64} (ray {r})" in msg


def test_prim_swapped_for_the_neighbouring_triangle_is_seen(want):
    i = _kept_ray(want, 4, 383 - 40)                   # in the last tile of the last pose
    got = _copy(want)
    got["prim"][i] ^= 1                                 # the other triangle of the same quad
    msg = _expect_failure(got, want, r"prim: 1 of 1920 rays differ; first at pose 4, tile 5 of the pose")
    assert "t:" not in msg and "rows:" not in msg


@pytest.mark.parametrize("field", ["point3", "normal3", "sem", "ins"])
def test_every_other_record_field_is_compared(want, field):
    i = _kept_ray(want, 1, 64)
    got = _copy(want)
    if field in ("sem", "ins"):
        got[field][i] += 1
    else:
        got[field].view(np.uint32)[i, 2] ^= 1
    msg = _expect_failure(got, want, rf"^planted: 1 of 1920 rays differ\n  {field}: 1 of 1920 rays differ; first at pose 1, tile 1 ")
    assert msg.count("\n") == 1


def test_a_removed_ray_reported_with_a_stale_field_is_seen(want):
    i = int(np.flatnonzero(~want["keep"])[7])
    got = _copy(want)
    got["point3"][i, 0] = 1.0                           # a miss must carry zeros
    _expect_failure(got, want, r"point3: 1 of 1920 rays differ")
    got = _copy(want)
    got["t"][i] = -np.inf
    _expect_failure(got, want, r"t: 1 of 1920 rays differ")


def test_two_exchanged_rows_are_seen_and_traced_to_their_rays(want):
    c = np.cumsum(want["counts"])
    r = int(c[2]) + 3                                   # rows 3 and 4 of pose 3
    got = _copy(want)
    got["rows"][[r, r + 1]] = got["rows"][[r + 1, r]]
    src = np.flatnonzero(want["keep"])[r]
    msg = _expect_failure(got, want, rf"rows: 2 of {len(want['rows'])} kept rows differ; first at row {r}, made from pose 3, ")
    assert f"(ray {src % N})" in msg and msg.startswith("planted: 2 of 1920 rays differ")


def test_a_label_bit_in_a_row_is_seen(want):
    got = _copy(want)
    got["rows"].view(np.uint32)[5, 3] ^= 1 << 16        # the instance half
    _expect_failure(got, want, r"rows: 1 of \d+ kept rows differ; first at row 5, made from pose 0")


def test_a_count_off_by_one_is_seen(want):
    got = _copy(want)
    got["counts"][3] += 1
    msg = _expect_failure(got, want, rf"counts: 1 of 5 poses differ; first at pose 3: got {want['counts'][3] + 1}, expected {want['counts'][3]}")
    assert "rows:" not in msg
    got = _copy(want)
    got["counts"] = got["counts"][:-1]
    _expect_failure(got, want, r"counts: 4 poses, expected 5")


def test_a_row_written_beyond_the_kept_ones_is_seen(want):
    K = len(want["rows"])
    got = _copy(want)
    got["rows"][K + 2, 1] = 0.0
    _expect_failure(got, want, rf"rows: 1 rows beyond the {K} kept ones were written; first at row {K + 2}")
    got = _copy(want)
    got["rows"] = got["rows"][:K - 1]                   # too few rows
    _expect_failure(got, want, rf"rows: {K - 1} rows, expected at least {K}")


def test_a_missing_or_misnamed_field_is_an_error_not_a_pass(want):
    got = _copy(want)
    del got["ins"]
    with pytest.raises(KeyError):
        fp.assert_scan_equal(got, want, "missing")
    with pytest.raises(KeyError):
        fp.assert_scan_equal(_copy(want), want, "misnamed", fields=("t", "primitive"))
    got = _copy(want)
    del got["fill"]
    with pytest.raises(KeyError):
        fp.assert_scan_equal(got, want, "no fill")
    got = _copy(want)
    got["sem"] = got["sem"].astype(np.int32)            # the right values in the wrong type
    _expect_failure(got, want, r"sem: dtype int32, expected uint16")


def test_the_report_line(want, capsys):
    line = fp.report("host", want)
    assert re.fullmatch(r"\[full parity\] host: rays compared 1920, kept share 0\.\d{5}, rays that differ 0", line)
    assert line in capsys.readouterr().out
