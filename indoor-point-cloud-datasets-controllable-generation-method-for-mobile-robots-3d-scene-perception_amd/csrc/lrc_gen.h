// lrc_gen.h -- the ray generators of trace_kernel<GEN, ..> (lidarcast.hip) by name, and what each of them implies, stated once
// for the kernel and for the host that launches it.  GEN stays an int with these values: the kernels' mangled names carry it.
#pragma once

constexpr int kGenRays = 0;            // explicit rays
constexpr int kGenPoses = 1;           // pose x direction table: the product's pose-batched scan
constexpr int kGenAngles = 2;          // pose x per-ray scan angles (dual-axis sensor, opt-in)
constexpr int kGenGrid = 3;            // host only: a grid scan (lrc_scan_grid_*); launch_trace turns it into kGenPoses -- the
                                       // per-ray kernel here, the packet kernel in the laboratory build
constexpr int kGenSweeps = 4;          // motion record x direction table x firing fractions (moving-sensor sweeps, opt-in)
constexpr int kGenNoisy = 5;           // kGenPoses with seeded range noise, angle jitter and dropout drawn per ray (opt-in)
constexpr int kGenEchoes = 6;          // pose x direction table x offset table: K sub-rays per beam in the G neighbouring lanes
                                       // of a group, reduced to at most E echoes per beam behind the traversal (opt-in;
                                       // lrc_echo.h)
constexpr int kGenMaterials = 7;       // kGenPoses with surface materials: a ray that meets glass or a mirror is continued from
                                       // its hit point, segment by segment, behind the first traversal (opt-in; lrc_material.h,
                                       // DESIGN.md section 5j)
constexpr int kGenNoisySweeps = 8;     // kGenSweeps with the seeded noise of kGenNoisy: the row is jittered in front of the dgemm
                                       // chain, the direction swept behind it (opt-in)

// rays come in the order of the direction table, pose by pose: the launch deals every pose's tiles to the XCDs in 16 chunks
constexpr bool gen_table_order(int gen) {
    return gen == kGenPoses || gen == kGenSweeps || gen == kGenNoisy || gen == kGenEchoes || gen == kGenMaterials ||
           gen == kGenNoisySweeps;
}
// waves per SIMD the register allocator leaves room for (the kernel's launch bounds): the table-order generators over the
// quantised node images run at eight, the material chain at six, the instrumented kernels wherever they come out
constexpr int gen_min_waves(int gen, int qn, bool stats) {
    return stats ? 1 : gen == kGenMaterials ? 6 : (qn != 0 && gen_table_order(gen)) ? 8 : 1;
}
// a pose of whole tiles gives the kernel tiles_per_pose: pose and in-pose index from the tile number
constexpr bool gen_pose_is_tiles(int gen) { return gen == kGenPoses || gen == kGenGrid; }
// the range-filter centre is formed from the motion record and the firing fraction, not fetched from a pose
constexpr bool gen_centre_from_motion(int gen) { return gen == kGenSweeps || gen == kGenNoisySweeps; }
// draws seeded noise in the kernel (p.noise); such a scan has refused a range_noise option
constexpr bool gen_draws_noise(int gen) { return gen == kGenNoisy || gen == kGenNoisySweeps; }
// the frames of such a scan are traced in ONE chunk: the columns that travel beside the record set are gathered from one
// packed run of compacted rows (echo_scan_compact, material_scan_compact)
constexpr bool gen_frames_one_chunk(int gen) { return gen == kGenEchoes || gen == kGenMaterials; }
// the laboratory build has measured alternatives of these only (kGenGrid has become kGenPoses by then)
constexpr bool gen_has_lab_variant(int gen) { return gen == kGenRays || gen == kGenPoses; }
