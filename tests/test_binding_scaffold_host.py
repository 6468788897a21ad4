"""CPU: the Python binding layer's outside -- the signature of every public callable of lidarcast.core and of RaycastEngineHIP
(recorded below; the helpers those layers share are private and may change, this list may not), the exception class and message
each table-driven engine method raises for a sensor without a pose-independent direction table, and the module-level helpers
of lidarcast.core that need no loaded library: the keep-mask conversion, the direction-table resolver, the side-tensor check."""
import inspect
import types

import numpy as np
import pytest

SIGNATURES = {
    "Context.__init__": "(self, device=0)",
    "Context.close": "(self)",
    "Context.cloud_from_ranges_dev": "(self, poses_t, dirs_t, t_label_t, out_rows_t, counts_t=None, stream=0)",
    "Context.cloud_range_stats_dev": "(self, rows_t, counts_t, range_t, mean_t, std_t, stream=0)",
    "Context.compact": "(self, t, seg_len, point3=None, sem=None, ins=None, incident_deg=None, want_index=False, want_xyzl=False)",
    "Context.compact_dev": "(self, nseg, seg_len, io, stream=0)",
    "Context.launch_chaining": "(self)",
    "Context.set_launch_chaining": "(self, enabled=True)",
    "Context.synchronize": "(self)",
    "DeviceHits.__init__": "(self, n, device, want=('t', 'prim', 'normal3', 'point3', 'sem', 'ins'))",
    "DeviceHits.bytes_per_ray": "(self)",
    "DirectionTable.__init__": "(self, ctx, dirs, fire=None)",
    "DirectionTable.close": "(self)",
    "DirectionTable.set_fire": "(self, fire)",
    "NearestIndex.__init__": "(self, ctx, points, cell_size=0.0)",
    "NearestIndex.close": "(self)",
    "NearestIndex.query": "(self, points, return_distance=False)",
    "NearestIndex.query_dev": "(self, q_t, idx_t, dist_t=None, stream=0)",
    "OccupancyIndex.__init__": "(self, ctx, vertices)",
    "OccupancyIndex.close": "(self)",
    "OccupancyIndex.occupied": "(self, points, half)",
    "PinnedPool.__init__": "(self, ctx, max_free_bytes=1073741824, max_outstanding_bytes=4294967296)",
    "PinnedPool.clear": "(self)",
    "PinnedPool.reserve": "(self, sizes)",
    "PinnedPool.take": "(self, nbytes)",
    "ScanPipe.__init__": "(self, scene, max_poses, rays_per_pose)",
    "ScanPipe.assemble": "(self, dirs_t, gathered, stream=0)",
    "ScanPipe.close": "(self)",
    "ScanPipe.gathered": "(all_poses_t, all_prims_t, all_tile_counts_t, poses_per_slab, slab_stride_bytes, own_slab, own_ticket, out_rows_t, counts_t=None, scan_slot=0)",
    "ScanPipe.records": "(self, ticket)",
    "ScanPipe.scan_gathered": "(self, dirs_t, gathered, stream=0)",
    "ScanPipe.set_line_width": "(self, line_width)",
    "ScanPipe.set_ray_table": "(self, enable)",
    "ScanPipe.set_tile_lines": "(self, lines)",
    "ScanPipe.submit": "(self, poses_t, dirs_t, max_range, io=None, out_rows_t=None, counts_t=None, stream=0)",
    "ScanPipe.submit_sharded": "(self, poses_t, dirs_t, max_range, send_prim_t, send_tile_count_t, assemble=None, stream=0)",
    "ScanPipe.trace_done": "(self, ticket, stream=0)",
    "ScanPipe.trace_ms": "(self, ticket)",
    "ScanPipe.wait": "(self, stream=0)",
    "Scene.__init__": "(self, ctx, vertices, triangles, tri_sem=None, tri_ins=None)",
    "Scene.cast": "(self, rays, center=None, max_range=inf, want=('t', 'prim', 'normal3', 'point3', 'sem', 'ins', 'incident_deg'))",
    "Scene.cast_dev": "(self, rays_t, hits, center=None, max_range=inf, stream=0)",
    "Scene.cast_segments": "(self, rays, seg_offsets, centers, max_range, want=('t', 'prim', 'normal3', 'point3', 'sem', 'ins', 'incident_deg'))",
    "Scene.close": "(self)",
    "Scene.cloud_from_prims_dev": "(self, poses_t, dirs_t, prim_t, out_rows_t, counts_t=None, tile_count_t=None, poses_per_slab=0, slab_stride_bytes=0, stream=0, own_slab=None, own_io=None)",
    "Scene.counters": "(self)",
    "Scene.export_array": "(self, name)",
    "Scene.export_bvh": "(self)",
    "Scene.from_device": "(cls, ctx, verts_t, tris_t, sem_t=None, ins_t=None)",
    "Scene.occupancy": "(self)",
    "Scene.reset_options": "(self)",
    "Scene.scan_angles_compact": "(self, poses, angles, keep, max_range, want=('point3', 'sem', 'ins'), capacity=None)",
    "Scene.scan_angles_dev": "(self, poses_t, angles_t, keep_t, hits, max_range, stream=0)",
    "Scene.scan_echoes_compact": "(self, poses, dirs, max_range, beam, want=('point3', 'sem', 'ins'), capacity=None)",
    "Scene.scan_echoes_dev": "(self, poses_t, dirs_t, hits, max_range, beam, weight_t=None, offsets_t=None, stream=0)",
    "Scene.scan_materials_compact": "(self, poses, dirs, max_range, materials, want=('point3', 'sem', 'ins'), capacity=None)",
    "Scene.scan_materials_dev": "(self, poses_t, dirs_t, hits, max_range, materials, bounces_t=None, surface_t=None, stream=0)",
    "Scene.scan_movers_compact": "(self, poses, dirs, max_range, movers, mover_poses, want=('point3', 'sem', 'ins'), capacity=None)",
    "Scene.scan_movers_dev": "(self, poses_t, dirs_t, hits, max_range, movers, mover_poses_t, mover_t=None, stream=0)",
    "Scene.scan_noisy_compact": "(self, poses, dirs, max_range, noise, want=('point3', 'sem', 'ins'), capacity=None)",
    "Scene.scan_noisy_dev": "(self, poses_t, dirs_t, hits, max_range, noise, stream=0)",
    "Scene.scan_poses": "(self, poses, dirs, max_range, want=('t', 'prim', 'normal3', 'point3', 'sem', 'ins', 'incident_deg'))",
    "Scene.scan_poses_compact": "(self, poses, dirs, max_range, want=('point3', 'sem', 'ins'), capacity=None, grid=None)",
    "Scene.scan_poses_dev": "(self, poses_t, dirs_t, hits, max_range, stream=0, grid=None)",
    "Scene.scan_rays_compact": "(self, rays, keep, centers, max_range, want=('point3', 'sem', 'ins'), capacity=None)",
    "Scene.scan_stats": "(self, poses, dirs, max_range)",
    "Scene.scan_sweeps_compact": "(self, motion, dirs, fire, max_range, want=('point3', 'sem', 'ins'), capacity=None)",
    "Scene.scan_sweeps_dev": "(self, motion_t, dirs_t, fire_t, hits, max_range, stream=0)",
    "Scene.set_options": "(self, min_range=0.0, range_noise=None, incident_mode=0)",
    "bake_triangle_labels": "(index, vertices, triangles, semantic, instance)",
    "motion_records": "(start_poses, end_poses)",
    "RaycastEngineHIP.__init__": "(self, verbose=False, device=0, max_cached_scenes=4, cache_check='sampled', prelock_bytes=None)",
    "RaycastEngineHIP.cast_rays": "(self, rays, mesh, center=None, max_range=inf, want=None)",
    "RaycastEngineHIP.clear_cache": "(self)",
    "RaycastEngineHIP.cloud_from_gather": "(self, g, intrinsics, padded_poses, mesh)",
    "RaycastEngineHIP.coverage_sets": "(self, intrinsics, poses, mesh, num_sets=None, set_of_pose=None, max_range=None, chunk_poses=None)",
    "RaycastEngineHIP.frame_objects": "(self, intrinsics, poses, mesh, max_range=None, chunk_poses=None)",
    "RaycastEngineHIP.lidar_intersect_mesh": "(self, lidar, mesh)",
    "RaycastEngineHIP.occupancy_grid": "(self, intrinsics, poses, mesh, voxel_size=0.05, origin=None, dims=None, min_returns=1, max_range=None, chunk_poses=None)",
    "RaycastEngineHIP.prim_gather": "(self, poses_local, rays_per_pose, dist, group=None)",
    "RaycastEngineHIP.rays_intersect_mesh": "(self, rays: numpy.ndarray, mesh)",
    "RaycastEngineHIP.scan_block_into": "(self, g, intrinsics, block_poses, mesh)",
    "RaycastEngineHIP.scan_echo_frames": "(self, intrinsics, poses, mesh, beam, want=('point3', 'sem', 'ins'))",
    "RaycastEngineHIP.scan_frames": "(self, intrinsics, poses, mesh, want=('point3', 'sem', 'ins'))",
    "RaycastEngineHIP.scan_frames_dual_axis": "(self, lidars, mesh, want=('point3', 'sem', 'ins'))",
    "RaycastEngineHIP.scan_frames_lidars": "(self, lidars, mesh, want=('point3', 'sem', 'ins'))",
    "RaycastEngineHIP.scan_lidars": "(self, lidars, mesh, want=('t', 'point3', 'incident_deg'))",
    "RaycastEngineHIP.scan_material_frames": "(self, intrinsics, poses, mesh, materials, want=('point3', 'sem', 'ins'))",
    "RaycastEngineHIP.scan_mover_frames": "(self, intrinsics, poses, mesh, movers, mover_poses, want=('point3', 'sem', 'ins'))",
    "RaycastEngineHIP.scan_noisy_frames": "(self, intrinsics, poses, mesh, noise, want=('point3', 'sem', 'ins'))",
    "RaycastEngineHIP.scan_poses": "(self, intrinsics, poses, mesh, want=('t', 'point3', 'incident_deg'))",
    "RaycastEngineHIP.scan_sweep_frames": "(self, intrinsics, start_poses, end_poses, mesh, want=('point3', 'sem', 'ins'), inputs=None)",
    "RaycastEngineHIP.scene_for": "(self, mesh)",
    "RaycastEngineHIP.select_views": "(self, intrinsics, candidate_poses, mesh, budget, target_ratio=None)",
    "RaycastEngineHIP.split_frames": "(frames, name)",
    "RaycastEngineHIP.surface_coverage": "(self, intrinsics, poses, mesh, max_range=None)",
    "RaycastEngineHIP.sweep_inputs": "(self, intrinsics, start_poses, end_poses)",
    "RaycastEngineHIP.torch_device": "(self)",
}


def public_signatures(owner, module, prefix=""):
    """{dotted name: str(signature)} of the public functions defined in ``module`` that ``owner`` (a module or a class) holds,
    ``__init__`` included, classes of the module entered."""
    out = {}
    for name, member in sorted(vars(owner).items()):
        if name.startswith("_") and name != "__init__":
            continue
        if isinstance(member, (staticmethod, classmethod)):
            member = member.__func__
        if inspect.isclass(member):
            if member.__module__ == module:
                out.update(public_signatures(member, module, prefix + name + "."))
        elif inspect.isfunction(member) and member.__module__ == module:
            out[prefix + name] = str(inspect.signature(member))
    return out


def test_public_signatures_are_the_recorded_ones():
    import lidarcast.core as core
    from raycast_engine.raycast_engine_hip import RaycastEngineHIP
    now = public_signatures(core, core.__name__)
    now.update(public_signatures(RaycastEngineHIP, RaycastEngineHIP.__module__, "RaycastEngineHIP."))
    assert sorted(now) == sorted(SIGNATURES), (sorted(set(now) ^ set(SIGNATURES)))
    changed = {k: (SIGNATURES[k], v) for k, v in now.items() if SIGNATURES[k] != v}
    assert not changed, changed


# ---- the engine's "sensor has a pose-independent direction table" check ---------------------------------------------------------------

NO_TABLE = {     # method -> (arguments after (intrinsics, poses), exception class, message)
    "scan_poses": (("mesh",), ValueError, "sensor has no pose-independent direction table"),
    "scan_frames": (("mesh",), ValueError, "sensor has no pose-independent direction table"),
    "scan_noisy_frames": (("mesh", "noise"), ValueError,
                          "seeded sensor noise needs a sensor with a pose-independent direction table"),
    "scan_echo_frames": (("mesh", "beam"), ValueError, "a beam footprint needs a sensor with a pose-independent direction table"),
    "scan_material_frames": (("mesh", "materials"), ValueError,
                             "surface materials need a sensor with a pose-independent direction table"),
    "scan_mover_frames": (("mesh", "movers", "mover_poses"), ValueError,
                          "moving objects need a sensor with a pose-independent direction table"),
    "sweep_inputs": ((np.eye(4)[None],), NotImplementedError,
                     "moving-sensor sweeps need a sensor with a pose-independent direction table"),
}


class _NoSceneEngine:
    """An engine that was never constructed (no context, no GPU): the check has to come before any scene is asked for."""

    def __new__(cls):
        from raycast_engine.raycast_engine_hip import RaycastEngineHIP

        class Probe(RaycastEngineHIP):
            def scene_for(self, mesh):
                raise AssertionError("the sensor check must come before the scene is built")

        return object.__new__(Probe)


@pytest.mark.parametrize("method", list(NO_TABLE))
@pytest.mark.parametrize("sensor", ["plain_object", "dual_axis"])
def test_engine_methods_refuse_a_sensor_without_direction_table(method, sensor):
    from lidar import DualAxisLidarIntrinsics
    k = object() if sensor == "plain_object" else DualAxisLidarIntrinsics()
    assert not hasattr(k, "horizontal_res") or hasattr(k, "swing_amplitude")
    args, exc, message = NO_TABLE[method]
    with pytest.raises(exc) as info:
        getattr(_NoSceneEngine(), method)(k, np.eye(4)[None], *args)
    assert type(info.value) is exc and str(info.value) == message


# ---- the module-level helpers of lidarcast.core (no library, no GPU) ----------------------------------------------------------------

def test_keep_mask_conversion():
    from lidarcast.core import _keep_mask
    P, N = 3, 5
    mask = np.random.default_rng(0).random((P, N)) < 0.5
    assert _keep_mask(None, P, N) is None
    as_view = _keep_mask(mask, P, N)
    assert as_view.dtype == np.uint8 and as_view.shape == (P, N) and np.shares_memory(as_view, mask)       # a view, no copy
    assert (as_view == mask).all() and set(np.unique(as_view)) <= {0, 1}
    u8 = mask.astype(np.uint8)
    assert np.shares_memory(_keep_mask(u8, P, N), u8)                   # already what the library reads
    for other in (mask.reshape(-1), np.asfortranarray(mask), mask.tolist(), mask.astype(np.int64), 7 * u8):
        got = _keep_mask(other, P, N)
        assert got.dtype == np.uint8 and got.shape == (P, N) and got.flags.c_contiguous
        assert ((got != 0) == mask).all()
    with pytest.raises(ValueError):
        _keep_mask(mask, P, N + 1)


def _stand_in_table(ctx, handle):
    """A DirectionTable that never met the library: the resolver looks at its handle and its context only."""
    from lidarcast import DirectionTable
    t = DirectionTable.__new__(DirectionTable)
    t.ctx, t._h, t.n, t.fire = ctx, handle, 4, None
    return t


def test_table_resolver_checks_and_hands_back_the_callers_table():
    from lidarcast.core import _table_for
    ctx, other = types.SimpleNamespace(_h=None), types.SimpleNamespace(_h=None)
    with pytest.raises(ValueError) as info:
        with _table_for(ctx, _stand_in_table(ctx, None)):
            raise AssertionError("a closed table was handed out")
    assert str(info.value) == "direction table handle is closed"
    with pytest.raises(ValueError) as info:
        with _table_for(ctx, _stand_in_table(other, 1234)):
            raise AssertionError("a table of another context was handed out")
    assert str(info.value) == "direction table belongs to another context (device)"
    mine = _stand_in_table(ctx, 1234)
    with _table_for(ctx, mine) as table:
        assert table is mine
    assert mine._h == 1234                                              # the caller's table is not closed behind its back
    with pytest.raises(RuntimeError, match="inside"):                   # nor when the scan raises
        with _table_for(ctx, mine):
            raise RuntimeError("inside")
    assert mine._h == 1234
    mine._h = None                                                      # (nothing for __del__ to destroy)


def test_table_resolver_closes_the_table_it_made(monkeypatch):
    import lidarcast.core as core
    made = []

    class Table:
        def __init__(self, ctx, dirs, fire=None):
            self.args, self.closed = (ctx, dirs, fire), 0
            made.append(self)

        def close(self):
            self.closed += 1

    monkeypatch.setattr(core, "DirectionTable", Table)
    with core._table_for("ctx", "dirs", "fire") as table:
        assert table is made[0] and table.args == ("ctx", "dirs", "fire") and table.closed == 0
    assert made[0].closed == 1
    with pytest.raises(RuntimeError, match="inside"):
        with core._table_for("ctx", "dirs"):
            raise RuntimeError("inside")
    assert len(made) == 2 and made[1].closed == 1 and made[1].args == ("ctx", "dirs", None)


def test_side_tensor_check():
    import torch
    from lidarcast.core import _check_side_tensor
    poses = torch.zeros((2, 16), dtype=torch.float64)                  # a CPU tensor: every side tensor is on the wrong device
    _check_side_tensor("x_t", None, torch.uint8, 6, "hold P * N entries", poses)
    with pytest.raises(ValueError, match="x_t must be torch.uint8"):
        _check_side_tensor("x_t", torch.zeros(6, dtype=torch.int32), torch.uint8, 6, "hold P * N entries", poses)
    with pytest.raises(ValueError, match="x_t must lie on the device of the poses"):
        _check_side_tensor("x_t", torch.zeros(6, dtype=torch.uint8), torch.uint8, 6, "hold P * N entries", poses)


def test_device_pointer_and_stream():
    import ctypes as C
    from lidarcast.core import _dptr, _stream
    assert _dptr(None) is None
    p = _dptr(types.SimpleNamespace(data_ptr=lambda: 0x7F0000001000))
    assert isinstance(p, C.c_void_p) and p.value == 0x7F0000001000
    assert isinstance(_stream(0), C.c_void_p) and _stream(0).value is None and _stream(0x1000).value == 0x1000
