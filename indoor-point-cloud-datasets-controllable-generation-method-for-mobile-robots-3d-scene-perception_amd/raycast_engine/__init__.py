"""Ray-cast engines behind the reference's engine interface.  ``RaycastEngineGPU`` and ``RaycastEngineCPU`` are both
the MI355X engine (there is no CPU compute path in this package); ``RaycastEngineBase`` is the abstract interface."""
from . import raycast_engine as _base
from . import raycast_engine_hip as _hip

RaycastEngineBase = _base.RaycastEngineBase
RaycastEngineHIP, RaycastEngineGPU, RaycastEngineCPU = _hip.RaycastEngineHIP, _hip.RaycastEngineGPU, _hip.RaycastEngineCPU
mesh_arrays = _hip.mesh_arrays
# scene flow under movers lives in lidarcast.flow, the engine as its first argument; bound here as the engines' method
from lidarcast.flow import scan_flow_frames as _scan_flow_frames  # noqa: E402
RaycastEngineHIP.scan_flow_frames = _scan_flow_frames
# ... and so does the seeded sensor noise under movers, in lidarcast.movers
from lidarcast.movers import scan_noisy_mover_frames as _scan_noisy_mover_frames  # noqa: E402
RaycastEngineHIP.scan_noisy_mover_frames = _scan_noisy_mover_frames
# ... and dynamic occupancy (per-frame grids under movers), in lidarcast.voxseq
from lidarcast.voxseq import dynamic_occupancy as _dynamic_occupancy  # noqa: E402
RaycastEngineHIP.dynamic_occupancy = _dynamic_occupancy

__all__ = ["RaycastEngineBase", "RaycastEngineCPU", "RaycastEngineGPU", "RaycastEngineHIP", "mesh_arrays"]
