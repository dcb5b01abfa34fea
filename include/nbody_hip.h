/*
 * nbody_hip.h -- C ABI of libnbody_hip.so, the MI355X (gfx950) force/integration engine.
 *
 * This is the drop-in boundary for the hot path of LessUp/n-body: every entry point
 * replaces one CUDA launch wrapper / class method of the reference (cited per
 * function as `ref: file:line`, paths relative to the reference checkout).  The
 * reference itself has no C ABI; its plugin API is the C++ strategy interface
 * `nbody::ForceCalculator` (include/nbody/force_calculator.hpp:36-89).  The C++
 * facade in n-body_amd/facade/ re-creates those classes on top of this header;
 * INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *  - plain pointers and sizes only; every `float*` inside nbody_particle_data is a
 *    DEVICE pointer (hipMalloc'd, caller-owned) unless the function says "host".
 *  - every call returns 0 on success or a negative nbody_hip_status; the message is
 *    available from nbody_hip_last_error() (thread-local), formatted like the
 *    reference's CudaException ("<what> at file:line", error_handling.hpp:29-51).
 *  - calls are asynchronous on the context's HIP stream unless they return a value
 *    to the host (energies) or say "blocking".  Not thread-safe per context, like
 *    the reference (force_calculator.hpp:8-19).
 *  - no CPU fallback exists: without a HIP device every entry point fails with
 *    NBODY_HIP_ERR_DEVICE.
 */
#ifndef NBODY_HIP_H
#define NBODY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NBODY_HIP_ABI_VERSION 1

/* exported with default visibility; everything else in the library is hidden */
#if defined(__GNUC__)
#define NBODY_HIP_API __attribute__((visibility("default")))
#else
#define NBODY_HIP_API
#endif

typedef enum nbody_hip_status {
  NBODY_HIP_OK = 0,
  NBODY_HIP_ERR_VALIDATION = -1, /* bad argument (ref: ValidationException) */
  NBODY_HIP_ERR_DEVICE = -2,     /* HIP runtime error (ref: CudaException) */
  NBODY_HIP_ERR_RESOURCE = -3,   /* out of memory / grid too large (ref: ResourceException) */
  NBODY_HIP_ERR_STATE = -4       /* call sequence error (NULL handle, not initialised) */
} nbody_hip_status;

/* ref: ForceMethod, include/nbody/types.hpp:66-70 (same enumerator order) */
typedef enum nbody_hip_force_method {
  NBODY_HIP_DIRECT_N2 = 0,
  NBODY_HIP_BARNES_HUT = 1,
  NBODY_HIP_SPATIAL_HASH = 2
} nbody_hip_force_method;

/*
 * ref: nbody::ParticleData, include/nbody/types.hpp:234-276.  Layout-identical
 * (13 float* then size_t count, 112 bytes), so a `nbody::ParticleData*` can be
 * passed straight through the boundary with a reinterpret_cast.
 */
typedef struct nbody_particle_data {
  float* pos_x; float* pos_y; float* pos_z;
  float* vel_x; float* vel_y; float* vel_z;
  float* acc_x; float* acc_y; float* acc_z;
  float* acc_old_x; float* acc_old_y; float* acc_old_z;
  float* mass;
  size_t count;
} nbody_particle_data;

/* 16-byte packed body used by the native (sharded / multi-GPU) entry points:
 * {x, y, z, mass}.  Accelerations use the same type with w unused. */
typedef struct nbody_float4 { float x, y, z, w; } nbody_float4;

typedef struct nbody_hip_ctx nbody_hip_ctx;

/* ---- library / context -------------------------------------------------- */

NBODY_HIP_API int nbody_hip_abi_version(void);
/* Which radix sort bins the bodies (Barnes-Hut build, spatial-hash build; the reference calls thrust::sort_by_key,
 * ref: src/cuda/force_barnes_hut.cu:276-280, force_spatial_hash.cu:286-288).  Above the crossover sizes one of
 *   - the library's driver of rocPRIM's Onesweep kernels (csrc/onesweep.h; compiled only for the rocPRIM version it was
 *     written against, and not with -DNBH_SORT_DRIVER=0: driver_compiled), the default while its run-time self-test holds (self_test: 0 = not run yet --
 *     no tree / grid made --, 1 = it reproduced the public sort word for word in this process, 2 = it did not: off);
 *   - the hand-written sort of csrc/radix_sort.h (no rocPRIM), which runs when the driver is absent or off, or with
 *     NBH_SORT=own in the environment (own_self_test: the same three states);
 * below them, with NBH_SORT=public, or when both are off: rocprim::radix_sort_pairs.  rocprim_version: ROCPRIM_VERSION of
 * the build.  Any pointer may be NULL. */
NBODY_HIP_API int nbody_hip_sort_info(int* driver_compiled, int* self_test, int* own_self_test, int* rocprim_version);
NBODY_HIP_API const char* nbody_hip_last_error(void);

/* Number of HIP devices visible (0 when there is no GPU; never fails). */
NBODY_HIP_API int nbody_hip_device_count(void);

/* Creates a context on `device`.  `stream` is a hipStream_t the caller owns; NULL means HIP's
 * default (null) stream, which is what the reference launches on (force_direct.cu:93).  The
 * context never creates streams of its own. */
NBODY_HIP_API int nbody_hip_ctx_create(nbody_hip_ctx** out, int device, void* stream);
NBODY_HIP_API int nbody_hip_ctx_destroy(nbody_hip_ctx* ctx);
/* Re-targets later launches to another caller-owned stream (NULL = the null stream). */
NBODY_HIP_API int nbody_hip_ctx_set_stream(nbody_hip_ctx* ctx, void* stream);
/* Blocks until all work queued on the context's stream is done.
 * ref: CUDA_CHECK_KERNEL's debug-mode cudaDeviceSynchronize, error_handling.hpp:124-136 */
NBODY_HIP_API int nbody_hip_ctx_synchronize(nbody_hip_ctx* ctx);

/* ---- step graphs (MI355X-native addition; no reference counterpart) ------------------------
 * Between capture_begin and capture_end every call made with this context is recorded into a
 * hipGraph instead of being executed; graph_launch replays the recording `times` times on the
 * context's stream (one host call for a whole run of steps).  Rules: run the same calls once
 * eagerly first (workspaces are sized on first use and allocation is not capturable); the pointers
 * and body count are baked into the recording; calls that return data to the host (energies,
 * *_info, *_stats, download, the spatial-hash grid build) are not capturable and fail with
 * NBODY_HIP_ERR_STATE, after which capture_end reports the failure and restores the context.
 * Measured (profiles/r01_step_graph_probe.txt): replay == eager time per step on MI355X, the
 * inter-kernel gaps being GPU-side; the gain is host CPU time, not step rate. */
typedef struct nbody_hip_graph nbody_hip_graph;
NBODY_HIP_API int nbody_hip_capture_begin(nbody_hip_ctx* ctx);
NBODY_HIP_API int nbody_hip_capture_end(nbody_hip_ctx* ctx, nbody_hip_graph** out);
NBODY_HIP_API int nbody_hip_graph_launch(nbody_hip_graph* graph, int times);
NBODY_HIP_API int nbody_hip_graph_destroy(nbody_hip_graph* graph);

/* ---- a11: particle memory (ref: ParticleDataManager, src/cuda/particle_init.cu:143-283) */

/* ref: allocateDevice :143-168 -- 13 arrays of `count` floats, accelerations zeroed.
 * One slab allocation, 256-byte aligned sub-arrays; freed by nbody_hip_particles_free. */
NBODY_HIP_API int nbody_hip_particles_alloc(nbody_particle_data* d, size_t count);
/* ref: freeDevice :170-198 -- frees and nulls every pointer, count = 0. */
NBODY_HIP_API int nbody_hip_particles_free(nbody_particle_data* d);
/* ref: copyToDevice :257-269 -- host -> device of pos, vel, acc, mass (10 arrays; acc_old is
 * NOT copied, as in the reference).  Blocking. */
NBODY_HIP_API int nbody_hip_particles_upload(nbody_particle_data* d, const nbody_particle_data* h);
/* ref: copyToHost :271-283 -- device -> host of the same 10 arrays.  Blocking. */
NBODY_HIP_API int nbody_hip_particles_download(nbody_particle_data* h, const nbody_particle_data* d);

/* ---- a4: Direct N^2 (ref: src/cuda/force_direct.cu:10-106) ---------------- */

/* ref: launchDirectForceKernel(ParticleData*, G, eps2, block_size) :88-98.
 * Reads pos_*, mass; OVERWRITES acc_* with a_i = G * sum_{j != i} m_j r_ij (|r_ij|^2+eps2)^-3/2.
 * `block_size` is accepted for signature parity and validated (1..1024) but does not pick the
 * launch shape: tiling is chosen for the 256-CU part from `count`. */
NBODY_HIP_API int nbody_hip_direct_forces(nbody_hip_ctx* ctx, const nbody_particle_data* d, float G, float eps2,
                            int block_size);

/* Native form used by the sharded (multi-GPU) path: accelerations of `n_targets` packed
 * bodies due to `n_sources` packed bodies (targets may be a sub-range of the sources; a
 * coincident pair contributes exactly zero, which is how the self pair is skipped).
 * acc_out[i] = {ax, ay, az, 0}.  If `accumulate` is non-zero the result is ADDED to acc_out
 * (used to overlap the local-shard pass with the all-gather of the remote shards). */
NBODY_HIP_API int nbody_hip_direct_forces_packed(nbody_hip_ctx* ctx, const nbody_float4* targets,
                                   size_t n_targets, const nbody_float4* sources,
                                   size_t n_sources, nbody_float4* acc_out, float G, float eps2,
                                   int accumulate);

/* Two DISJOINT body sets a and b, every a x b pair evaluated ONCE (Newton's third law):
 * acc_a (+)= forces on a from b, acc_b (+)= forces on b from a.  The sharded path uses it so that
 * a pair of shards is computed by one rank only; the reactions travel back in a reduce-scatter.
 * Needs eps2 >= 1e-12. */
NBODY_HIP_API int nbody_hip_direct_forces_pair_packed(nbody_hip_ctx* ctx, const nbody_float4* a, size_t n_a,
                                                      const nbody_float4* b, size_t n_b, nbody_float4* acc_a,
                                                      int accumulate_a, nbody_float4* acc_b, int accumulate_b,
                                                      float G, float eps2);

/* SoA <-> packed conversion on device (x,y,z,mass -> float4 and back). */
NBODY_HIP_API int nbody_hip_pack_posm(nbody_hip_ctx* ctx, const float* x, const float* y, const float* z,
                        const float* mass, size_t count, nbody_float4* out);
NBODY_HIP_API int nbody_hip_unpack3(nbody_hip_ctx* ctx, const nbody_float4* in, size_t count, float* x,
                      float* y, float* z);

/* ---- a6: Velocity Verlet (ref: src/cuda/integrator.cu:11-48,122-152,224-238) */

/* ref: launchUpdatePositionsKernel :122-131   x += v dt + a (dt^2/2) */
NBODY_HIP_API int nbody_hip_update_positions(nbody_hip_ctx* ctx, nbody_particle_data* d, float dt);
/* ref: launchUpdateVelocitiesKernel :133-142  v += (a_old + a) (dt/2) */
NBODY_HIP_API int nbody_hip_update_velocities(nbody_hip_ctx* ctx, nbody_particle_data* d, float dt);
/* ref: launchStoreAccelerationsKernel :144-152  a_old = a */
NBODY_HIP_API int nbody_hip_store_accelerations(nbody_hip_ctx* ctx, nbody_particle_data* d);
/* storeOldAccelerations + updatePositions in one pass (what Integrator::integrate does first,
 * integrator.cu:224-231): a_old <- a ; x += v dt + a dt^2/2.  Same arithmetic, one launch instead of four. */
NBODY_HIP_API int nbody_hip_drift(nbody_hip_ctx* ctx, nbody_particle_data* d, float dt);
/* ref: Integrator::integrate with a DirectForceCalculator :224-238, `steps` times:
 * one fused drift pass (a_old<-a, x update, float4 pack), the force kernel, and the
 * velocity update fused into the force reduction epilogue. */
NBODY_HIP_API int nbody_hip_integrate_direct(nbody_hip_ctx* ctx, nbody_particle_data* d, float G, float eps2,
                               float dt, int steps);

/* Packed (float4) halves of the same step for the sharded multi-GPU path, where each rank
 * keeps only its target range: drift = x += v dt + a dt^2/2 on {x,y,z,m}; kick =
 * v += (a_old + a_new) dt/2.  The caller swaps its two acceleration buffers between steps
 * (no a_old copy).  ref: integrator.cu:16-19 and :31-34. */
NBODY_HIP_API int nbody_hip_drift_packed(nbody_hip_ctx* ctx, nbody_float4* posm, const nbody_float4* vel,
                                         const nbody_float4* acc, size_t count, float dt);
NBODY_HIP_API int nbody_hip_kick_packed(nbody_hip_ctx* ctx, nbody_float4* vel, const nbody_float4* acc_old,
                                        const nbody_float4* acc_new, size_t count, float dt);

/* ---- a7: energies (ref: src/cuda/integrator.cu:51-119,252-293) ------------ */

/* ref: Integrator::computeKineticEnergy :252-269 -- 0.5 sum m v^2.  fp64 reduction on device,
 * result rounded to float like the reference's return type.  Blocking. */
NBODY_HIP_API int nbody_hip_kinetic_energy(nbody_hip_ctx* ctx, const nbody_particle_data* d, float* out);
/* ref: Integrator::computePotentialEnergy :271-289 -- -G sum_{i<j} m_i m_j / sqrt(r^2+eps^2).
 * Takes eps (not eps^2) like the reference.  Blocking. */
NBODY_HIP_API int nbody_hip_potential_energy(nbody_hip_ctx* ctx, const nbody_particle_data* d, float G,
                               float eps, float* out);
/* fp64 variants of the two above (no final rounding to float). */
NBODY_HIP_API int nbody_hip_kinetic_energy_f64(nbody_hip_ctx* ctx, const nbody_particle_data* d, double* out);
NBODY_HIP_API int nbody_hip_potential_energy_f64(nbody_hip_ctx* ctx, const nbody_particle_data* d, float G,
                                   float eps, double* out);

/* e (SURVEY 8e "KE/PE via all-reduce of one fp64"): energies of ONE SHARD of a sharded run.
 * out[0] = sum over the targets of 0.5 m v^2; out[1] = -G/2 sum_{i in targets} m_i sum_{j in sources,
 * j != self_offset + i} m_j / sqrt(r_ij^2 + eps^2): target i is source number self_offset + i (for
 * disjoint sets pass self_offset >= n_sources or <= -n_targets, so that no target maps to a source).  Summed over a partition of the
 * bodies (each rank: its shard against the gathered bodies) the two numbers are the system's KE
 * and PE as nbody_hip_*_energy_f64 computes them.  Same per-term fp32 arithmetic, fp64 sums. */
NBODY_HIP_API int nbody_hip_energies_packed(nbody_hip_ctx* ctx, const nbody_float4* targets_posm,
                                            const nbody_float4* targets_vel, size_t n_targets,
                                            long long self_offset, const nbody_float4* sources_posm,
                                            size_t n_sources, float G, float eps, double out[2]);

/* ---- a9: spatial hash (ref: SpatialHashGrid / SpatialHashCalculator,
 *          src/cuda/force_spatial_hash.cu:14-377, include/nbody/spatial_hash_grid.hpp:9-59) ---- */

typedef struct nbody_hip_grid nbody_hip_grid;

/* ref: SpatialHashGrid(max_particles, cell_size) :155-168.  Sized once from `max_particles`
 * (the reference sizes its grid from the first count it sees, :372-374). */
NBODY_HIP_API int nbody_hip_grid_create(nbody_hip_ctx* ctx, size_t max_particles, float cell_size,
                                        nbody_hip_grid** out);
NBODY_HIP_API int nbody_hip_grid_destroy(nbody_hip_grid* grid);
/* ref: SpatialHashCalculator::setCellSize (force_calculator.hpp:199): takes effect at the next build */
NBODY_HIP_API int nbody_hip_grid_set_cell_size(nbody_hip_grid* grid, float cell_size);
/* Tuning hook for measurements: force kernel 0 = automatic, 1 = cell-run kernel (one workgroup per
 * run of cells along x, binary-searched ranges; the only one for very sparse grids), 2 / 3 / 4 = wave-per-
 * cell kernel with 1 / 2 / 4 bodies per lane (needs a grid of at most ~4 cells per body).  All give the
 * reference's 27-cell result; they differ by fp rounding of the summation order only.
 * 6 = two bodies per lane with the window filtered by the box of the cell's bodies (automatic from 8 bodies per cell
 *     when cutoff <= cell_size, from 40 when cutoff > cell_size);
 * 7 = two-phase form of the wave-per-cell kernel (distance masks first; measured, not the default);
 * 8 = one lane per body (automatic below 8 bodies per cell), 9 = its split form (8 for the cells of few bodies, 3 for
 *     the crowded ones: automatic from 500,000 bodies), 10 = two bodies of one cell per lane (measured: 7-17 % faster
 *     than 8 between 3 and 9 bodies per cell, bound by the L1 path; not chosen automatically);
 * 5 = TIMING PROBE, not a force kernel: the wave-per-cell kernel over the half shell (own cell + 13 forward
 * neighbours) without reactions -- a lower bound for the time of a Newton's-third-law variant;
 * its output is meaningless. */
NBODY_HIP_API int nbody_hip_grid_tuning(nbody_hip_grid* grid, int kernel);
/* ref: SpatialHashGrid::build :235-303 -- bounding box (padded 0.001), grid dims
 * ceil(extent/cell)+1, cell id per body, bodies ordered by cell.  More than 1e8 cells ->
 * NBODY_HIP_ERR_RESOURCE ("Spatial hash grid too large", :252-254).  One host round trip
 * (the grid size), like the reference. */
NBODY_HIP_API int nbody_hip_grid_build(nbody_hip_grid* grid, const nbody_particle_data* d);
/* nbody_hip_drift + nbody_hip_grid_build in one pass over the bodies (see nbody_hip_tree_drift_build); used by
 * Integrator::integrate for exactly the engine's own SpatialHashCalculator. */
NBODY_HIP_API int nbody_hip_grid_drift_build(nbody_hip_grid* grid, nbody_particle_data* d, float dt);
/* ref: SpatialHashGrid::computeForces(d_particles, cutoff, G, eps) :305-316 -- takes eps and
 * cutoff unsquared like the reference; OVERWRITES acc_*. */
NBODY_HIP_API int nbody_hip_grid_compute_forces(nbody_hip_grid* grid, nbody_particle_data* d,
                                                float cutoff, float G, float eps);
/* ref: getGridDims / getTotalCells (spatial_hash_grid.hpp:20-24) + the padded bounding box. */
NBODY_HIP_API int nbody_hip_grid_info(const nbody_hip_grid* grid, int dims[3], int* total_cells,
                                      float bbox_min[3], float bbox_max[3]);
/* Number of bodies of the last build (0 before the first): the length of the per-body arrays
 * copy_cell_data writes (the reference keeps it as the ParticleData count it was built from). */
NBODY_HIP_API int nbody_hip_grid_count(const nbody_hip_grid* grid, size_t* built_count);
/* ref: copyCellDataToHost :318-331 -- HOST output arrays (any may be NULL): cell_start/cell_end
 * [total_cells] (0/0 for an empty cell), particle_cells [count], sorted_indices [count].
 * Blocking. */
NBODY_HIP_API int nbody_hip_grid_copy_cell_data(nbody_hip_grid* grid, int* cell_start, int* cell_end,
                                                int* particle_cells, int* sorted_indices);

/* Packed forms used by the sharded (multi-GPU, z-slab) spatial-hash path.  `bounds` = {lo x,y,z,
 * hi x,y,z} of the ALREADY PADDED global box (NULL: box of these bodies padded by 0.001), so that
 * every rank bins on the same grid; acc_out[i] = {ax, ay, az, 0} for every body of the last build,
 * in its input order (a rank passes [own bodies; halo bodies] and keeps the first part). */
NBODY_HIP_API int nbody_hip_grid_build_packed(nbody_hip_grid* grid, const nbody_float4* posm, size_t count,
                                              const float* bounds);
NBODY_HIP_API int nbody_hip_grid_compute_forces_packed(nbody_hip_grid* grid, float cutoff, float G, float eps,
                                                       nbody_float4* acc_out);
/* Bodies [first, first + count) of the last build in CELL ORDER (x fastest, then y, then z: a z layer
 * is one contiguous run), copied to a DEVICE array.  The sharded step takes a rank's lowest and highest
 * layer from here: they are the halo its neighbours need.  Asynchronous. */
NBODY_HIP_API int nbody_hip_grid_sorted_bodies(nbody_hip_grid* grid, size_t first, size_t count, nbody_float4* out);
/* e3 (multi-GPU spatial hash; no reference counterpart): the z layers [z_first, z_first + z_count) of the
 * global grid are the only ones later nbody_hip_grid_build_packed calls WITH explicit bounds put bodies
 * in (a rank's slab, or its slab plus the two halo layers): the per-cell start array of the force kernel
 * then covers just those layers.  z_count <= 0 (default): the whole grid. */
NBODY_HIP_API int nbody_hip_grid_set_slab(nbody_hip_grid* grid, int z_first, int z_count);
/* Forces on the bodies of `targets` that lie in the layers [z_first, z_first + z_count) (z_count <= 0:
 * all) from the bodies of `sources` -- another grid built on the SAME global box and cell size, or the
 * same grid.  acc_out has one row per body of `targets` in its input order; only the rows of the bodies
 * in those layers are written (accumulate != 0: added to).  The sharded step evaluates own x own while
 * the halo layers are in flight, then boundary layers x halo with accumulate.  Both grids must be dense
 * enough to carry a per-cell start array (NBODY_HIP_ERR_STATE otherwise: use the one-grid path). */
NBODY_HIP_API int nbody_hip_grid_forces_pair_packed(nbody_hip_grid* targets, nbody_hip_grid* sources, int z_first,
                                                    int z_count, float cutoff, float G, float eps,
                                                    nbody_float4* acc_out, int accumulate);

/* The boundary pass of a z-slab decomposition without a second grid (round 4).  A rank's own grid (packed build with
 * nbody_hip_grid_set_slab) can hand one of its z layers to a neighbour READY FOR USE: nbody_hip_grid_export_layer writes
 * the layer's bodies in cell order (as many as the layer holds) and its start array rebased to 0 (dims[0] * dims[1] + 1
 * ints).  nbody_hip_grid_forces_layer_packed evaluates the targets of layer z of `grid` against such a layer (which is
 * layer src_z of the same global grid: same origin, dimensions, cell size), adding to acc_out when accumulate != 0.
 * Same pair set and arithmetic as the 27-cell search of ref: src/cuda/force_spatial_hash.cu:104-146 restricted to the
 * source layer's cells. */
NBODY_HIP_API int nbody_hip_grid_export_layer(nbody_hip_grid* grid, int z, nbody_float4* bodies_out, int* lb_out);
NBODY_HIP_API int nbody_hip_grid_forces_layer_packed(nbody_hip_grid* grid, int z, const nbody_float4* src_bodies,
                                                     const int* src_lb, int src_z, float cutoff, float G, float eps,
                                                     nbody_float4* acc_out, int accumulate);
/* Inspection of what the force kernels read (tests; both blocking, HOST outputs).
 * The per-cell start array of the last build: has_array = 0 when the grid was too sparse to get one (more than
 * 16 cells per body + 4096, or an empty slab), else 1 with the cells [lb_base, lb_base + lb_count] it covers --
 * the whole grid, or the slab of nbody_hip_grid_set_slab clipped to the grid -- and lb_out[c - lb_base] = number of
 * bodies OF THE BUILD whose cell id is below c (lb_count + 1 ints).  Bodies in layers outside the slab are counted
 * like any other: the entries stay lower bounds over all sorted bodies.  Any pointer may be NULL (lb_out = NULL
 * asks for the size).  Changes no state. */
NBODY_HIP_API int nbody_hip_grid_copy_cell_lb(nbody_hip_grid* grid, int* has_array, int* lb_base, int* lb_count,
                                              int* lb_out);
/* The work list the wave-per-cell kernels take, made from the start array of the last build for the cells
 * [cell_first, cell_end) exactly as a force call makes it (the same list call: the grid's alternating counters move
 * on).  mode 0: units only; 1: cells below min_cnt bodies put their bodies' sorted positions on the `light` list
 * instead; 2: the same in pairs (sorted position of the first of two bodies of a cell, top bit on a cell's last, odd
 * one).  A unit is {cell - cell_first, chunk index}, ceil(bodies / chunk) of them per cell of at least min_cnt bodies.
 * units_out [capacity][2]: the units of the cells above 48 bodies in the slots [0, counts[0]), the others in
 * [capacity - counts[2], capacity), each group in no particular order, the slots between unspecified.  counts_out:
 * {units in front, bodies of the most crowded cell if above 64 else 0, units at the back, entries of `light`};
 * light_out [counts[3]] (room for one int per body of the build; modes 1, 2).  units_out = NULL only reports
 * capacity_out and runs nothing.  No start array: NBODY_HIP_ERR_STATE; a range that is empty or not inside
 * [lb_base, lb_base + lb_count]: NBODY_HIP_ERR_VALIDATION. */
NBODY_HIP_API int nbody_hip_grid_unit_list(nbody_hip_grid* grid, long long cell_first, long long cell_end, int chunk,
                                           int min_cnt, int mode, int* units_out, int* light_out, int counts_out[4],
                                           int* capacity_out);
/* One partition pass of a rank's bodies after the drift (csrc/slab.hip).  gbox_dev: DEVICE array
 * {min x,y,z, max x,y,z} of ALL ranks' bodies (the all-reduced nbody_hip_bbox_packed result, unpadded);
 * the global grid is derived from it on the device exactly as SpatialHashGrid::build does (ref:
 * force_spatial_hash.cu:225-246).  Layer z belongs to rank ((z + 1) world - 1) / gz.  Outputs, all DEVICE:
 *   rows_out        the bodies that CHANGE OWNER, 16 floats each {x,y,z,m | vx,vy,vz,0 | ax,ay,az,0 |
 *                   id,z,0,0 (int bits)}, grouped by new owner (ascending, own rank absent), each group in
 *                   input order; capacity n rows
 *   holes_out       the input positions of those bodies, ascending; capacity n ints
 *   send_matrix_dev world x world ints, zeroed, row `rank` = bodies per new owner, entry [rank][rank] = the
 *                   bodies that stay (sum over ranks = who sends how many rows to whom)
 *   hist_dev        hist_cap ints: this rank's bodies per layer (sum over ranks = population of every
 *                   layer, hence every rank's new body count and the size of its halo layers); zero from
 *                   layer gz on.  When gz > hist_cap the first hist_cap layers are still counted.
 *   info_dev        4 ints: gx, gy, gz, and 1 if gz > hist_cap (the caller must fall back)
 * The bodies that stay are not touched.  Asynchronous; gid may be NULL (ids = input positions); with
 * world == 1 rows_out / holes_out may be NULL.  rows_out and holes_out are written up to the number of
 * leavers and not beyond.  world may be up to 64 here and in nbody_hip_slab_layer_owner (the width of the
 * pass: one ballot per owner, owners kept in a byte); the sharded systems of nbody_hip_comm.h stop at
 * NBODY_HIP_MAX_RANKS = 32, so nothing in this library calls the pass with more.
 * Pinned bit for bit by tests/test_slab_gpu.py against tests/slab_ref.py. */
NBODY_HIP_API int nbody_hip_slab_partition(nbody_hip_ctx* ctx, const nbody_float4* posm, const nbody_float4* vel,
                                           const nbody_float4* acc, const int* gid, size_t n, const float* gbox_dev,
                                           float cell_size, int world, int rank, int hist_cap, float* rows_out,
                                           int* holes_out, int* send_matrix_dev, int* hist_dev, int* info_dev);
/* The same with the ranks' slabs bounded by PHYSICAL z coordinates: z_cuts = world - 1 ascending HOST floats (NULL:
 * equal layer counts, as above); the owner of a layer is the number of cuts at or below the layer's centre,
 * nbody_hip_slab_layer_owner -- the same arithmetic on the device and on the host, so that every rank's host can
 * derive the ranks' layer ranges.  A host that balances the slabs by body count picks the cuts from the (all-reduced)
 * layer histogram of the previous evaluation. */
NBODY_HIP_API int nbody_hip_slab_partition_cuts(nbody_hip_ctx* ctx, const nbody_float4* posm, const nbody_float4* vel,
                                                const nbody_float4* acc, const int* gid, size_t count,
                                                const float* gbox_device, float cell_size, int world, int rank,
                                                int hist_cap, float* rows_out, int* holes_out, int* send_matrix_device,
                                                int* hist_device, int* info_device, const float* z_cuts);
NBODY_HIP_API int nbody_hip_slab_layer_owner(int layer, float lo_z, float cell_size, int world, const float* z_cuts);
/* After the exchange: n_old bodies (arrays with room for n_old - n_holes + n_arrivals) of which the slots
 * holes[0..n_holes) (ascending, as written by the partition) are vacant, and n_arrivals rows received from
 * the other ranks -> the n_new = n_old - n_holes + n_arrivals bodies of the rank, contiguous from slot 0.
 * The order is part of the contract (a sharded run is bitwise reproducible only because of it):
 *   arrival t goes into holes[t]; once the holes are used up, into slot n_old + (t - n_holes);
 *   with fewer arrivals than holes, the bodies of the old tail [n_new, n_old) that are not holes themselves,
 *   taken in ASCENDING slot order, go into holes[n_arrivals], holes[n_arrivals + 1], ... in ASCENDING order
 *   (exactly as many as there are such holes below n_new).
 * Every other slot below n_new keeps its body; nothing is written past max(n_old, n_new); the slots
 * [n_new, n_old) keep what they held.  Moves 64 bytes per migrating body and nothing else.  All four words of
 * a row's velocity and acceleration quadruples are copied (the partition writes 0 there).  gid may be NULL. */
NBODY_HIP_API int nbody_hip_slab_fill(nbody_hip_ctx* ctx, const float* rows, size_t n_arrivals, const int* holes,
                                      size_t n_holes, size_t n_old, nbody_float4* posm, nbody_float4* vel,
                                      nbody_float4* acc, int* gid);
/* min/max of packed bodies into a DEVICE array of 6 floats {lo x,y,z, hi x,y,z} (async; the ranks
 * all-reduce it).  ref: computeBoundingBoxKernel, force_barnes_hut.cu:66-110 */
NBODY_HIP_API int nbody_hip_bbox_packed(nbody_hip_ctx* ctx, const nbody_float4* posm, size_t count,
                                        float* bounds_device);
/* The float4 drift of nbody_hip_drift_packed (x += v dt + a dt^2/2, integrator.cu:16-19) and the box of the NEW
 * positions in ONE pass.  enc_device: 6 words private to the caller that hold the empty box {0xffffffff x3, 0 x3}
 * before the FIRST call; every call leaves them re-armed.  Async. */
NBODY_HIP_API int nbody_hip_drift_bbox_packed(nbody_hip_ctx* ctx, nbody_float4* posm, const nbody_float4* vel,
                                              const nbody_float4* acc, size_t count, float dt,
                                              unsigned int* enc_device, float* bounds_device);
/* z cell coordinate (clamped to [0, gz-1]) of packed bodies on a grid with origin lo_z; DEVICE
 * int output.  ref: assignCellsKernel, force_spatial_hash.cu:28-49 */
NBODY_HIP_API int nbody_hip_cell_z_packed(nbody_hip_ctx* ctx, const nbody_float4* posm, size_t count,
                                          float lo_z, float cell_size, int gz, int* cz_device);

/* ---- a8: Barnes-Hut (ref: BarnesHutTree / BarnesHutCalculator,
 *          src/cuda/force_barnes_hut.cu:204-532, include/nbody/barnes_hut_tree.hpp:9-81) ---- */

typedef struct nbody_hip_tree nbody_hip_tree;

/* Tuning hook for measurements: number of replicas (power of two, <= 16) that share each wave's
 * walk when there are few bodies, and the number of ownership units per replica (a unit is a subtree
 * of at most n / (units K) bodies; default: n / 96 whatever K); 0 = automatic.
 * Results are deterministic for a given setting; different settings differ by fp rounding only. */
NBODY_HIP_API int nbody_hip_tree_tuning(nbody_hip_tree* tree, int replicas, int units_per_replica);

/* Form of the walk without replicas: 1 = plain (one sibling node per step), 2 = pair walk (two sibling nodes per
 * packed instruction, node records as pair blocks; same interaction lists, a sibling group's fp32 sum formed as
 * (even siblings) + (odd siblings)), its waves scheduled longest-first from the node visits the previous walk
 * recorded; 3 = pair walk in plain order; 0 = automatic (2).  Results do not depend on the schedule.
 * The pair walk needs the even-aligned node ids a build gives trees of >= 98,304 bodies (smaller trees are walked with
 * replicas of the plain walk and keep plain ids); to force it on a smaller tree set the form BEFORE the build -- asking
 * for it afterwards fails with NBODY_HIP_ERR_STATE. */
NBODY_HIP_API int nbody_hip_tree_walk_form(nbody_hip_tree* tree, int form);
/* Test / stress hook: cap the node arrays at `max_nodes` (0 = the bound on the node count; the arrays also stop
 * at 2^28 - 1 nodes, the width of a child link).  A tree that would need more nodes is cut where the numbering
 * passes the capacity: the nodes beyond do not exist and their parents are leaves of several bodies, which interact
 * body by body -- forces stay correct (closer to the direct sum than the full tree's), the walk gets slower. */
NBODY_HIP_API int nbody_hip_tree_limit_nodes(nbody_hip_tree* tree, int max_nodes);
/* Node-visit counting for nbody_hip_tree_stats (off by default: it costs a memset launch and an
 * atomic per wave in every walk). */
NBODY_HIP_API int nbody_hip_tree_count_visits(nbody_hip_tree* tree, int enable);

/* Diagnostics of the last walk made with visit counting on: out[p] (p = 0..64) = internal-node tests made
 * with p lanes of the wave taking part, out[65 + q] = with q lanes accepting the node's monopole.
 * Blocking. */
NBODY_HIP_API int nbody_hip_tree_visit_histogram(nbody_hip_tree* tree, unsigned long long out[130]);

/* ref: BarnesHutTree(max_particles) :204-210 */
NBODY_HIP_API int nbody_hip_tree_create(nbody_hip_ctx* ctx, size_t max_particles, nbody_hip_tree** out);
NBODY_HIP_API int nbody_hip_tree_destroy(nbody_hip_tree* tree);
/* Tree shape: levels below the root (1..21; default 20, the depth the reference's insertion loop stops
 * at, :363) and the largest body count a leaf may hold (default 1, as in the reference, where a leaf
 * holds one particle; at the deepest level a leaf keeps whatever falls into its cell).  Up to 10 levels
 * the bodies are ordered by the reference's 30-bit Morton code (:23-38) in 32-bit keys; deeper trees use
 * 63-bit keys (21 bits per axis, a refinement of the same grid).  Re-sizes the key, flag and node arrays;
 * the tree must be rebuilt afterwards. */
NBODY_HIP_API int nbody_hip_tree_set_params(nbody_hip_tree* tree, int max_depth, int leaf_max);
/* ref: BarnesHutTree::build :282-289 -- bounding box, Morton keys, sort, octree, monopoles; all on
 * the device, no host round trip (the reference crosses PCIe >= 17 times here). */
NBODY_HIP_API int nbody_hip_tree_build(nbody_hip_tree* tree, const nbody_particle_data* d);
/* The drift of a Velocity-Verlet step (ref: Integrator::integrate, integrator.cu:224-238 -- storeOldAccelerations +
 * updatePositions: a_old <- a ; x += v dt + a dt^2/2) fused with the build that follows it: the positions are
 * advanced, packed and bounded in ONE pass over the bodies, then the tree is built on them.  Same arithmetic and
 * results as nbody_hip_drift followed by nbody_hip_tree_build.  Used by Integrator::integrate for exactly the
 * engine's own BarnesHutCalculator (a subclass goes through its virtual computeForces). */
NBODY_HIP_API int nbody_hip_tree_drift_build(nbody_hip_tree* tree, nbody_particle_data* d, float dt);
/* ref: BarnesHutTree::computeForces(d_particles, theta, G, eps) :488-498 -- OVERWRITES acc_*. */
NBODY_HIP_API int nbody_hip_tree_compute_forces(nbody_hip_tree* tree, nbody_particle_data* d,
                                                float theta, float G, float eps);

/* e (multi-GPU Barnes-Hut: replicated tree, partitioned walk; no reference counterpart).
 * build_packed: the same build from float4 {x, y, z, m} bodies (the gathered bodies of all ranks).
 * compute_forces_packed: walks only the bodies at positions [first_sorted, first_sorted + count) of
 * the tree's Morton-sorted order and writes their accelerations as {ax, ay, az, 0} at the bodies'
 * ORIGINAL indices of acc_out (n float4, rows of other bodies untouched).  Ranks that walk disjoint
 * ranges of the same tree produce, together, exactly the single-GPU result. */
NBODY_HIP_API int nbody_hip_tree_build_packed(nbody_hip_tree* tree, const nbody_float4* posm, size_t n);
NBODY_HIP_API int nbody_hip_tree_compute_forces_packed(nbody_hip_tree* tree, size_t first_sorted, size_t count,
                                                       float theta, float G, float eps, nbody_float4* acc_out);
/* ref: getNodeCount (barnes_hut_tree.hpp:41) and the root mass used by verifyMassConservation
 * (:511-519); plus node visits (per wave) of the last traversal and the first node id of every
 * level: level_base[l] for l = 0 .. max_depth + 1 (the last one = node count), repeated up to
 * NBODY_HIP_TREE_LEVELS entries (trees go down to depth 21; the deepest level that holds nodes is what
 * the reference's getMaxDepth reports).  Any output may be NULL.  Blocking. */
#define NBODY_HIP_TREE_LEVELS 24
NBODY_HIP_API int nbody_hip_tree_stats(nbody_hip_tree* tree, int* node_count, float* root_mass,
                                       unsigned long long* nodes_visited, int level_base[NBODY_HIP_TREE_LEVELS]);
/* The node ids of the last build as the walks use them (nbody_hip_tree_stats and nbody_hip_tree_copy_nodes report the
 * compacted numbering, without holes): *aligned = 1 if the sibling groups were padded to even ids (the pair walk's
 * numbering), 0 for plain ids; id_base[l] = first id of level l for l = 0 .. max_depth + 1 (the last one = ids in use,
 * holes included), repeated like level_base above.  Either output may be NULL.  Blocking. */
NBODY_HIP_API int nbody_hip_tree_id_layout(nbody_hip_tree* tree, int* aligned, int id_base[NBODY_HIP_TREE_LEVELS]);
/* ref: copyNodesToHost / getNodes :500-503 -- writes the tree into HOST memory in the reference's
 * OctreeNode layout (76 bytes, barnes_hut_tree.hpp:9-30), children indexed by octant; optionally
 * the Morton order (sorted position -> body index, `count` ints).  Blocking. */
NBODY_HIP_API int nbody_hip_tree_copy_nodes(nbody_hip_tree* tree, void* host_nodes, int capacity_nodes,
                                            int* sorted_indices);

/* e (no reference counterpart): MULTIPOLE ORDER of the tree's walk, 1 (default: monopoles, the reference's model) or 2
 * (monopoles + quadrupoles).  At order 2 every build also computes the second moment of every node about its centre
 * of mass, S = sum_k m_k (y_k - c)(y_k - c)^T (fp64 on the device, bottom-up by the parallel-axis theorem, stored in
 * fp32; allocated at the first order-2 build), and an ACCEPTED internal node of mass M and centre c acts on a body at
 * x, with d = c - x and h = |d|^2 + eps^2, as the second-order Taylor expansion of the Plummer-softened kernel:
 *   a   = G [ M d h^-3/2 - 3 S d h^-5/2 - 3/2 tr(S) d h^-5/2 + 15/2 (d^T S d) d h^-7/2 ]
 *   phi = -G [ M h^-1/2 + 3/2 (d^T S d) h^-5/2 - 1/2 tr(S) h^-3/2 ]            (grad phi = -a exactly)
 * The opening test, the self-skip and the leaves (one-body leaves exact, leaves of several bodies body by body) are
 * those of order 1, so every body's interaction list is the order-1 list; the force error falls about one power of
 * theta faster.  Order 2 walks with the plain walk whatever nbody_hip_tree_walk_form says (its
 * results do not depend on that setting) and honours replicas and visit counting; compute_forces,
 * compute_forces_packed and potential all use the order of the LAST BUILD.
 * set: 1 or 2, anything else ERR_VALIDATION; takes effect at the next build -- a walk or potential call on a tree whose
 *      order changed since its last build fails with ERR_STATE.  The first order-2 build cannot be recorded into a step
 *      graph (it allocates).  get: the order set.
 * copy_moments: 6 floats per node (Sxx, Syy, Szz, Sxy, Sxz, Syz) into HOST memory in the node numbering of
 *      nbody_hip_tree_copy_nodes; ERR_STATE on a tree not built at order 2, ERR_VALIDATION when capacity_nodes is
 *      below the node count.  Blocking. */
NBODY_HIP_API int nbody_hip_tree_set_multipole_order(nbody_hip_tree* tree, int order);
NBODY_HIP_API int nbody_hip_tree_get_multipole_order(nbody_hip_tree* tree, int* order);
NBODY_HIP_API int nbody_hip_tree_copy_moments(nbody_hip_tree* tree, float* host, int capacity_nodes);

/* e (no reference counterpart): PER-BODY POTENTIAL of each force method, in that method's own model, and
 * PE = 1/2 sum_i m_i phi_i.
 *   direct: phi_i = -G sum_{j != i} m_j / sqrt(r_ij^2 + eps^2)  (every ordered pair; a coincident pair with
 *           eps = 0 contributes nothing, as in energy above)
 *   tree:   the same sum over exactly the interaction list of nbody_hip_tree_compute_forces on the tree as last
 *           built, for the same theta, eps, G: accepted nodes -G M / sqrt(d^2 + eps^2), leaves body by body
 *   grid:   the truncated potential SHIFTED to zero at the cutoff over exactly the pair set of
 *           nbody_hip_grid_compute_forces on the grid as last built (27 cells, unsoftened r^2 < cutoff^2):
 *           -G sum_j m_j (1 / sqrt(r^2 + eps^2) - 1 / sqrt(cutoff^2 + eps^2)) -- the energy a hash run conserves
 * phi: DEVICE array of d->count floats in the original body order; pe: HOST double, summed in fp64 from the per-body
 * fp64 sums in a fixed order (bitwise reproducible).  Either may be NULL, not both.  Take eps (not eps^2) like the
 * energy calls.  Write no acc_* / acc_old_* and leave the tree's walk schedule and the grid's statistics alone; the
 * result does not depend on any tuning, walk form or deterministic mode.  Not capturable; blocking when pe is asked
 * for.  Errors as the matching compute_forces (not built / count mismatch: ERR_STATE; theta outside [0, 2], a cutoff
 * that is not positive and finite: ERR_VALIDATION). */
NBODY_HIP_API int nbody_hip_direct_potential(nbody_hip_ctx* ctx, const nbody_particle_data* d, float G, float eps,
                                             float* phi, double* pe);
NBODY_HIP_API int nbody_hip_tree_potential(nbody_hip_tree* tree, const nbody_particle_data* d, float theta, float G,
                                           float eps, float* phi, double* pe);
NBODY_HIP_API int nbody_hip_grid_potential(nbody_hip_grid* grid, const nbody_particle_data* d, float cutoff, float G,
                                           float eps, float* phi, double* pe);

/* e (no reference counterpart): ACCELERATION AND POTENTIAL AT ARBITRARY POINTS, in each method's own model.  A point is
 * never "a body": nothing is skipped by index, and the bodies feel nothing of the points.
 * points: DEVICE array of n_points {x, y, z, ignored}; out: DEVICE array of n_points {ax, ay, az, phi} in the caller's
 * point order.  Take eps (not eps^2) like the potential calls.
 *   direct: a(x) = G sum_j m_j (r_j - x) (|r_j - x|^2 + eps^2)^-3/2, phi(x) = -G sum_j m_j (|r_j - x|^2 + eps^2)^-1/2 over
 *           all bodies of d.  A body coincident with the point adds zero force and -G m_j / eps to phi -- except with
 *           eps^2 < 1e-12 (the guard convention of the force kernels), where it contributes nothing to either.
 *   tree:   the interaction list the opening test of nbody_hip_tree_compute_forces gives the position x on the tree as
 *           last built (same distance chain, same `size2 < theta^2 dist2` form), WITHOUT a self-skip: accepted nodes by
 *           their multipoles, leaves body by body.  The multipole order is that of the last build; order 2 uses the
 *           formulas of nbody_hip_tree_set_multipole_order for a and phi.  Points outside the tree's bounding box are
 *           legal (every node is further away, nothing else changes).
 *   grid:   the point's cell is the grid's own clamped cell coordinate against the box and cell size of the last build;
 *           the pair set is the 27-cell window of that cell, a pair counting when the unsoftened fp32 r^2 (the force
 *           kernels' fma chain) is below fl(cutoff * cutoff) -- and above 0 with eps^2 < 1e-12.  a is the truncated
 *           force, phi the shifted truncated potential of nbody_hip_grid_potential.  For cutoff <= cell size this is
 *           the truncated sum over ALL bodies wherever the point lies, outside the box included (a point further than
 *           the cutoff from every body gets exact zeros); for a larger cutoff it is the 27-cell model, as for the bodies.
 * Every row is a function of its point and the structure alone: all three calls are bitwise invariant under a permutation
 * of the points and from call to call; tree and grid also under splitting the points across several calls.  Direct
 * chooses its source splits from the POINT COUNT of the call, so its rows may differ in the last bit between calls of
 * different sizes.  A non-finite point yields a row of NaN, for that point only.
 * Write no acc_* / acc_old_*; leave the walk schedule, the visit counters and the grid's statistics alone; ignore every
 * tuning, walk form and deterministic mode.  Asynchronous on the context's stream.  Not capturable into a step graph (the
 * first call allocates point workspace on the handle, later ones may grow it).  n_points == 0 succeeds and does nothing.
 * More than 2^30 points in one call: NBODY_HIP_ERR_RESOURCE (the kernels index points with 32-bit integers).
 * Errors as the matching compute_forces: a tree / grid that is not built, or a tree whose multipole order changed since
 * its build: ERR_STATE; null points or out, theta outside [0, 2], a cutoff that is not positive and finite:
 * ERR_VALIDATION. */
NBODY_HIP_API int nbody_hip_direct_field(nbody_hip_ctx* ctx, const nbody_particle_data* d, const nbody_float4* points,
                                         size_t n_points, float G, float eps, nbody_float4* out);
NBODY_HIP_API int nbody_hip_tree_field(nbody_hip_tree* tree, const nbody_float4* points, size_t n_points, float theta,
                                       float G, float eps, nbody_float4* out);
NBODY_HIP_API int nbody_hip_grid_field(nbody_hip_grid* grid, const nbody_float4* points, size_t n_points, float cutoff,
                                       float G, float eps, nbody_float4* out);

/* e (no reference counterpart): DIRECT FORCE AND JERK, and the FOURTH-ORDER HERMITE INTEGRATOR on top of it.  The
 * reference integrates with Velocity Verlet only (ref: src/cuda/integrator.cu:224-238); Direct summation is the method
 * of collisional dynamics, whose codes integrate with the Hermite scheme, which needs the time derivative of the
 * acceleration from the same pair loop.  With d = r_j - r_i, w = v_j - v_i, h = |d|^2 + eps^2:
 *   a_i = G sum_j m_j d h^-3/2         j_i = da_i/dt = G sum_j m_j [ w - 3 (d.w)/h d ] h^-3/2
 * by the conventions of nbody_hip_direct_forces' one-sided kernel: the self pair contributes zero to both sums, a
 * coincident pair of two distinct bodies zero to a and m_j w / eps^3 to j (with eps^2 < 1e-12, the guard convention,
 * zero to both); fp32 sums of 256 sources folded into fp64, the source splits added in a fixed order, G applied in fp64.  No atomics in the sums: every result is bitwise reproducible from call to
 * call.  All calls take eps (not eps^2).
 * One step of size dt is the PEC form of Makino & Aarseth (1992), state in fp32, predictor and corrector evaluated in
 * fp64 from it and rounded once:
 *   xp = x + v dt + a dt^2/2 + j dt^3/6        vp = v + a dt + j dt^2/2                      (predict)
 *   (a1, j1) = the sums above at (xp, vp)                                                    (one N^2 sweep)
 *   v1 = v + (a + a1) dt/2 + (j - j1) dt^2/12  x1 = x + (v + v1) dt/2 + (a - a1) dt^2/12     (correct)
 * After a step acc_* = a1 and acc_old_* = a, as after a Velocity-Verlet step; j1 stays on the handle.  a1 and j1 belong
 * to the PREDICTED state: a run continued from a saved state primes (a, j) afresh at the corrected state, so it agrees
 * with the uninterrupted run to truncation order, NOT bit for bit (unlike nbody_hip_integrate_direct).
 * Errors: a null handle / particle data / array: ERR_STATE; count 0 or above max_particles, a dt that is not positive
 * ("Time step must be positive") or not finite ("Time step must be a finite number"), steps < 1, eps < 0, particle data
 * on another device than the context: ERR_VALIDATION.  None of the calls can be recorded into a step graph (the handle
 * allocates at first use). */
typedef struct nbody_hip_hermite nbody_hip_hermite;
/* An integrator for up to max_particles bodies on the context (16 bytes per body, allocated at the first priming; 24
 * more in extended state precision, below). */
NBODY_HIP_API int nbody_hip_hermite_create(nbody_hip_ctx* ctx, size_t max_particles, nbody_hip_hermite** out);
/* Waits for the context's stream, frees the handle.  A runtime that is already gone is answered with OK. */
NBODY_HIP_API int nbody_hip_hermite_destroy(nbody_hip_hermite* h);
/* (a, j) at the current x, v: OVERWRITES acc_*, keeps j on the handle, marks it primed.  Asynchronous on the context's
 * stream. */
NBODY_HIP_API int nbody_hip_hermite_prime(nbody_hip_hermite* h, nbody_particle_data* d, float G, float eps);
/* The caller changed x, v, m, G or eps behind the handle: the next step primes again.  (A step also primes again by
 * itself when count, G, eps or the pos_x pointer differ from those of the last priming.) */
NBODY_HIP_API int nbody_hip_hermite_invalidate(nbody_hip_hermite* h);
/* `steps` >= 1 Hermite steps of size dt queued back to back on the context's stream, no host synchronisation; primes
 * first if the handle is not primed.  Three launches per step; updates pos_*, vel_*, acc_*, acc_old_*. */
NBODY_HIP_API int nbody_hip_hermite_step(nbody_hip_hermite* h, nbody_particle_data* d, float G, float eps, float dt,
                                         int steps);
/* The jerk of the last evaluation, {jx, jy, jz, 0} per body in the caller's body order, copied to a DEVICE array of
 * `count` rows.  Asynchronous on the context's stream.  ERR_STATE if the handle is not primed. */
NBODY_HIP_API int nbody_hip_hermite_jerk(nbody_hip_hermite* h, nbody_float4* out_device);
/* The standard start-up time step eta * min_i |a_i| / |j_i| over the bodies with |j_i| > 0 of the last evaluation
 * (+inf when there is none), reduced on the device with it.  The integrator never changes dt itself.  Blocking;
 * ERR_STATE if the handle is not primed. */
NBODY_HIP_API int nbody_hip_hermite_suggest_dt(nbody_hip_hermite* h, float eta, float* out);
/* Standalone evaluation at the bodies: jerk_out[i] = {jx, jy, jz, 0} and, when acc_out is given, acc_out[i] =
 * {ax, ay, az, 0} with acc_* NOT written; with acc_out == NULL acc_* are overwritten.  DEVICE arrays of d->count rows.
 * Asynchronous on the context's stream. */
NBODY_HIP_API int nbody_hip_direct_acc_jerk(nbody_hip_ctx* ctx, nbody_particle_data* d, float G, float eps,
                                            nbody_float4* acc_out_or_null, nbody_float4* jerk_out);

/* EXTENDED STATE PRECISION of the two Hermite integrators (opt-in; the default, fp32, keeps every bit).  With an fp32
 * state the pair loop forms d = x_j - x_i from rounded positions: its relative error is 2^-24 |x| / |d|, which ruins a
 * tight pair that sits away from the origin, and the rounding of x and v after every step is the accuracy floor of the
 * scheme.  In extended mode the state of body i is the double-single pair
 *   X = pos + pos_lo,   V = vel + vel_lo,
 * pos_* / vel_* of the particle data the fp32 roundings (hi), the fp32 residuals (lo) on the integrator's handle (24 more
 * bytes per body, allocated at the first switch).  Invariant after every call: hi = (float)X, lo = (float)(X - hi), so the
 * particle data means what it means in fp32 mode; its layout and the checkpoint format are unchanged (a run continued
 * from a checkpoint restarts from the rounded state).  (X there is the fp64 value the corrector formed.  lo can round to
 * exactly half an ulp of hi, and hi + lo is then a tie between hi and its neighbour: pos_* / vel_* are the hi parts, do not
 * recover them by rounding hi + lo.)
 *   predictor, corrector   the fp64 expressions above evaluated from hi + lo (an exact fp64 sum) and rounded to hi + lo
 *                          instead of to fp32: v1 first, then x1 from that v1.  In the block scheme all bodies are
 *                          predicted so, each over its own h_i.  a and j stay fp32: acc_*, acc_old_* and the jerk on the
 *                          handle keep their meaning; the level rules and suggest_dt (which see a and j only) are unchanged.
 *   pair sweep             sources carry {xp_hi, m}, {vp_hi, 0} and {xp_lo, 0};
 *                          d = (x_j,hi - x_i,hi) + (x_j,lo - x_i,lo) in fp32, in that association (the hi difference is
 *                          exact for close pairs); w from the hi parts only.  Everything else is the sweep above: self
 *                          pair, coincident pairs (a pair whose hi parts coincide while the lo parts differ is a DISTINCT
 *                          pair), the guard, padding, 256-source fp32 tiles folded into fp64, fixed split order, no
 *                          atomics -- bitwise reproducible.  With all residuals zero the sums equal the fp32 mode's bit
 *                          for bit.
 * mode: 0 fp32 (default), 1 extended; another value: ERR_VALIDATION.  A switch unprimes the handle; switching to 1 starts
 * with residuals 0.  nbody_hip_hermite_invalidate in extended mode ALSO zeroes the residuals (the caller changed the
 * state: the fp32 arrays are the truth); the re-priming a step does by itself for another G or eps keeps them. */
NBODY_HIP_API int nbody_hip_hermite_set_precision(nbody_hip_hermite* h, int mode);
NBODY_HIP_API int nbody_hip_hermite_get_precision(nbody_hip_hermite* h, int* mode);
/* X and V from HOST arrays [count][3] in fp64: hi into the particle data, lo onto the handle (fp32 mode: the rounded
 * state only); unprimes.  Exact to the hi + lo representation (|X - (hi + lo)| <= 2^-49 |X|).  Blocking. */
NBODY_HIP_API int nbody_hip_hermite_set_state_f64(nbody_hip_hermite* h, nbody_particle_data* d, const double* pos_host,
                                                  const double* vel_host);
/* hi + lo in fp64 into HOST arrays [count][3] (fp32 mode: the arrays widened).  Blocking. */
NBODY_HIP_API int nbody_hip_hermite_get_state_f64(nbody_hip_hermite* h, nbody_particle_data* d, double* pos_host,
                                                  double* vel_host);
/* nbody_hip_direct_acc_jerk at the positions pos + pos_lo: pos_lo_device[i] = {lx, ly, lz, 0}, a DEVICE array of
 * d->count rows. */
NBODY_HIP_API int nbody_hip_direct_acc_jerk_ext(nbody_hip_ctx* ctx, nbody_particle_data* d,
                                                const nbody_float4* pos_lo_device, float G, float eps,
                                                nbody_float4* acc_out_or_null, nbody_float4* jerk_out);

/* f (no reference counterpart): the Hermite integrator above with INDIVIDUAL BLOCK TIME STEPS.  With one shared step
 * the one hard binary of a cluster sets the step of every body; here every body has its own, a power-of-two fraction
 * of the step of the call, chosen by the Aarseth criterion.  Direct-only, opt-in; nbody_hip_hermite_* is not changed.
 *
 * Time and levels.  One call advances the system by MACRO STEPS dt_max and ends with every body at the same time, so
 * the particle data means at every call boundary what it means after nbody_hip_hermite_step.  Body i steps with
 * dt_i = dt_max 2^-k_i, its level k_i in 0..L (L = max_level, default 16, at most 20).  Time inside a macro step is an
 * integer tick in [0, 2^L]; tick_i is the time of body i's last correction and a multiple of 2^(L - k_i).  INSIDE a macro
 * step pos_*, vel_*, acc_* of body i and its jerk on the handle are its state AT tick_i -- the bodies are not
 * synchronised until the macro step is complete.
 * Priming evaluates (a, j) at the state as nbody_hip_hermite_prime does, sets want_i = eta_start |a_i| / |j_i| (+inf when
 * |j_i| = 0), k_i to the smallest level with dt_max 2^-k <= want_i clamped to [0, L], and every tick to 0.
 * One BLOCK STEP:
 *   1. t = min_i (tick_i + 2^(L - k_i)); the active set is A = { i : tick_i + 2^(L - k_i) = t }.
 *   2. ALL bodies are predicted to t over h_i = (t - tick_i) dt_max / 2^L (formed in fp64) with the predictor above.
 *   3. (a1, j1) of the bodies of A over all N predicted sources, by the pair conventions above (self pair zero,
 *      coincident pair m w / eps^3 to j, guard convention below eps^2 = 1e-12, fp32 partial sums folded into fp64, splits
 *      in a fixed order, G in fp64, no floating-point atomics: bitwise reproducible).  Two kernel forms, chosen from the
 *      size of A (nbody_hip_hermite_block_tuning); each is reproducible, they differ from each other in the last bits.
 *   4. The bodies of A are corrected with their own h_i = dt_i by the corrector above; acc_old <- a, acc <- a1, j <- j1,
 *      tick_i <- t.  A body outside A has NONE of its arrays written.
 * New level of a corrected body, with a0, j0 the old and a1, j1 the new values and h its step (fp32 values in fp64):
 *   a2 = (-6 (a0 - a1) - h (4 j0 + 2 j1)) / h^2     a3 = (12 (a0 - a1) + 6 h (j0 + j1)) / h^3     a2 <- a2 + h a3
 *   want = sqrt(eta (|a1| |a2| + |j1|^2) / (|j1| |a3| + |a2|^2)), +inf when the denominator is 0
 *   want < dt_i: k is raised while want < dt_max 2^-k and k < L (any number of halvings; a level L that is still too
 *   long counts as a FLOOR HIT); else want >= 2 dt_i, k > 0 and t a multiple of 2 2^(L - k): k <- k - 1 (one doubling).
 * The macro step is complete when every tick equals 2^L, which the alignment rule guarantees is reached; the ticks are
 * then re-based to 0.  With max_level = 0 every body is active in every block step, the launch shape is that of
 * nbody_hip_hermite_step, and the run equals it bit for bit.
 * The state is fp32: below eta ~ 0.01 the rounding of the state, not the truncation of the scheme, bounds the accuracy
 * (DESIGN.md section 4.10).  Continuation after save / load: as for nbody_hip_hermite_step.
 * The host reads {t, |A|} back once per block step (8 bytes) to size the launches: every step and advance call
 * BLOCKS, and none of the calls can be recorded into a step graph -- unless the block steps are scheduled on the device
 * (nbody_hip_hermite_block_set_scheduling below, for small systems).
 * Errors: as nbody_hip_hermite_* (null handle / particle data / array: ERR_STATE; count 0 or above max_particles, the
 * dt_max wording "Time step must be positive" / "Time step must be a finite number", a step count < 1, eps < 0, data
 * on another device: ERR_VALIDATION).  A step or advance whose dt_max, G, eps, count or pos_x pointer differ from the
 * primed ones primes again when the handle is at tick 0, and fails with ERR_STATE in the middle of a macro step. */
typedef struct nbody_hip_hermite_block nbody_hip_hermite_block;
typedef struct nbody_hip_hermite_block_info_t {
  unsigned long long block_steps;      /* block steps since the last priming */
  unsigned long long body_steps;       /* corrected bodies summed over them: the sum of |A| */
  unsigned long long level_steps[21];  /* body steps by the level they were taken at */
  unsigned long long floor_hits;       /* corrections after which level max_level was still too long */
  unsigned long long narrow_launches;  /* block steps that took the narrow / the wide force-and-jerk kernel */
  unsigned long long wide_launches;
  unsigned long long macro_steps;      /* completed macro steps since the last priming */
  unsigned int current_tick;           /* 0 at a macro boundary */
  unsigned int last_n_active;          /* |A| of the last block step */
  int max_level;                       /* L of the last priming (before it: of the next) */
  int narrow_below;                    /* the crossover in effect: active sets smaller than it take the narrow form */
} nbody_hip_hermite_block_info_t;
/* An integrator for up to max_particles bodies on the context (32 bytes per body, allocated at the first priming). */
NBODY_HIP_API int nbody_hip_hermite_block_create(nbody_hip_ctx* ctx, size_t max_particles,
                                                 nbody_hip_hermite_block** out);
/* Waits for the context's stream, frees the handle.  A runtime that is already gone is answered with OK. */
NBODY_HIP_API int nbody_hip_hermite_block_destroy(nbody_hip_hermite_block* h);
/* eta and eta_start positive and finite, max_level in [0, 20]; defaults 0.02, 0.01, 16.  Take effect at the NEXT priming
 * (never in the middle of a macro step). */
NBODY_HIP_API int nbody_hip_hermite_block_set_params(nbody_hip_hermite_block* h, float eta, float eta_start,
                                                     int max_level);
/* (a, j) at the current x, v, the start levels for macro steps of dt_max, all ticks 0, the counters 0: OVERWRITES acc_*.
 * Asynchronous on the context's stream. */
NBODY_HIP_API int nbody_hip_hermite_block_prime(nbody_hip_hermite_block* h, nbody_particle_data* d, float G, float eps,
                                                float dt_max);
/* The caller changed x, v, m, G or eps behind the handle: the next call primes again (and starts a new macro step). */
NBODY_HIP_API int nbody_hip_hermite_block_invalidate(nbody_hip_hermite_block* h);
/* Up to block_steps >= 1 single block steps; stops early at a macro boundary.  Blocking (host scheduling). */
NBODY_HIP_API int nbody_hip_hermite_block_step(nbody_hip_hermite_block* h, nbody_particle_data* d, float G, float eps,
                                               float dt_max, int block_steps);
/* To the next macro_steps >= 1 macro boundaries: afterwards all bodies are synchronised.  Equals the same number of
 * calls with macro_steps = 1, and the matching sequence of nbody_hip_hermite_block_step calls, bit for bit.  Blocking
 * (host scheduling). */
NBODY_HIP_API int nbody_hip_hermite_block_advance(nbody_hip_hermite_block* h, nbody_particle_data* d, float G, float eps,
                                                  float dt_max, int macro_steps);
/* Per-body state into HOST arrays of `count` elements, any of which may be NULL: the levels, the ticks, want (what the
 * criterion asked for at the body's last correction or at priming) and the jerk {jx, jy, jz, 0} at tick_i.  Blocking;
 * ERR_STATE if the handle is not primed. */
NBODY_HIP_API int nbody_hip_hermite_block_state(nbody_hip_hermite_block* h, int* levels, unsigned int* ticks, float* want,
                                                nbody_float4* jerk);
/* Test / expert hook: replaces the levels (a HOST array of `count` values in [0, max_level]).  Only at tick 0 of a
 * primed handle (ERR_STATE otherwise); a level outside the range: ERR_VALIDATION. */
NBODY_HIP_API int nbody_hip_hermite_block_set_levels(nbody_hip_hermite_block* h, const int* levels_host);
/* Active sets smaller than narrow_below take the narrow kernel form: 0 automatic (the measured crossover; a block step
 * with every body active always takes the wide form, the shape of nbody_hip_hermite_step), 1 always wide, a value above
 * the body count always narrow. */
NBODY_HIP_API int nbody_hip_hermite_block_tuning(nbody_hip_hermite_block* h, int narrow_below);
/* The counters above.  Blocking (two of them live on the device). */
NBODY_HIP_API int nbody_hip_hermite_block_info(nbody_hip_hermite_block* h, nbody_hip_hermite_block_info_t* out);
/* Extended state precision, as for nbody_hip_hermite_* above (56 bytes per body in extended mode).  Switching the mode
 * or setting the state in the middle of a macro step: ERR_STATE.  nbody_hip_hermite_block_invalidate in extended mode
 * also zeroes the residuals; a re-priming for another G, eps or dt_max keeps them.  The info struct is unchanged:
 * get_precision is the query for the mode. */
NBODY_HIP_API int nbody_hip_hermite_block_set_precision(nbody_hip_hermite_block* h, int mode);
NBODY_HIP_API int nbody_hip_hermite_block_get_precision(nbody_hip_hermite_block* h, int* mode);
NBODY_HIP_API int nbody_hip_hermite_block_set_state_f64(nbody_hip_hermite_block* h, nbody_particle_data* d,
                                                        const double* pos_host, const double* vel_host);
NBODY_HIP_API int nbody_hip_hermite_block_get_state_f64(nbody_hip_hermite_block* h, nbody_particle_data* d,
                                                        double* pos_host, double* vel_host);
/* Where the block steps are scheduled.  The host form above costs five launches and one 8-byte read per block step
 * whatever it corrects, which is what a small system (a binary with a perturber, a planetary system, a cluster core)
 * spends its time on.  In the RESIDENT form one launch of ONE workgroup runs whole block steps back to back -- t, the
 * prediction, the active set, the sweep, the corrector, the levels -- until the macro boundary (advance: one launch per
 * macro step) or until its budget is used up (step: one launch; it stops early at the boundary as above).  The model is
 * the one above, word for word.  The sweep is the narrow kernel form's, so a resident run equals the host-scheduled run
 * with nbody_hip_hermite_block_tuning(h, 1 << 30) bit for bit: particle data, residuals, jerk, levels, ticks, want and
 * the counters (narrow_launches / wide_launches count host-form launches only).  DESIGN.md section 4.12.
 * mode 0: host scheduling (default; every step / advance BLOCKS, none can be recorded)
 *      1: resident, required: a step / advance with more than NBODY_HIP_HERMITE_BLOCK_RESIDENT_MAX bodies fails with
 *         ERR_VALIDATION
 *      2: automatic: resident when count < NBODY_HIP_HERMITE_BLOCK_RESIDENT_BELOW (the measured crossover), else host
 * A resident step / advance with the primed dt_max, G, eps, count and arrays is ASYNCHRONOUS and reads nothing from the
 * device; on a handle that has run once with these parameters it can be recorded into a step graph (a call that would
 * prime or allocate during a capture: ERR_STATE).  The schedule then lives on the device: info, set_levels,
 * set_precision, set_state_f64, set_scheduling and a step / advance with other parameters wait for the stream and read
 * it first; the rules above then apply (other parameters prime again at tick 0 and fail with ERR_STATE in the middle of
 * a macro step).  A launch that meets a schedule that cannot be (no active body, t not ahead of the current tick or
 * beyond 2^L) writes a status word and stops, the launches queued behind it return at once, and the next call that
 * reads the schedule fails with ERR_STATE ("block-step schedule out of range") and unprimes the handle.
 * set_scheduling in the middle of a macro step: ERR_STATE; at a boundary it keeps the priming and the counters.  A mode
 * outside 0..2: ERR_VALIDATION. */
#define NBODY_HIP_HERMITE_BLOCK_RESIDENT_MAX 4096
#define NBODY_HIP_HERMITE_BLOCK_RESIDENT_BELOW 0
NBODY_HIP_API int nbody_hip_hermite_block_set_scheduling(nbody_hip_hermite_block* h, int mode);
/* mode: the setting; last_form: what the last step / advance call ran (-1 none since the priming, 0 host, 1 resident). */
NBODY_HIP_API int nbody_hip_hermite_block_get_scheduling(nbody_hip_hermite_block* h, int* mode, int* last_form);

/* ---- block-step Hermite ENSEMBLES: many independent small systems per launch (no reference counterpart) ----
 *
 * One small system fills one of the GPU's 256 compute units at best; people run thousands of them (scattering
 * experiments, planetary systems drawn from a distribution, one cluster under many seeds).  The ensemble handle
 * advances B independent systems, stored back to back in ONE nbody_particle_data, with one workgroup per system in one
 * launch.  The model is the one above, word for word, applied to each system separately:
 *   - system s is the bodies [offsets[s], offsets[s+1]); sizes may differ, each is in
 *     [1, NBODY_HIP_HERMITE_BLOCK_RESIDENT_MAX]; no pair is formed across systems;
 *   - G, eps, eta, eta_start, max_level and the state precision are shared; dt_max is per system;
 *   - after advance(macro_steps) system s stands at macro_steps dt_max[s] and all its bodies are synchronised.
 * System s of an ensemble run equals the single-system handle above in resident scheduling (mode 1) on those bodies
 * alone, with the same parameters and number of macro steps, BIT FOR BIT: particle data, residuals, jerk, levels, ticks,
 * want and the counters.  It depends on nothing but that system: not on its place in the batch, not on the workgroup or
 * compute unit that ran it, not on the other systems.
 *
 * Call sequence: create, set_params / set_precision, set_layout, prime, advance ... ; info / state read back.
 * set_layout: offsets_host has n_systems + 1 entries with offsets[0] = 0, strictly ascending, every size in [1, 4096],
 * n_systems in [1, max_systems], the last offset at most max_particles_total; a violation is ERR_VALIDATION with a
 * message that names the system.  A new layout unprimes the handle.  Blocking (it uploads the layout; the only call
 * that allocates: 96 bytes per body of capacity at the first layout, 24 more in extended mode, and the sweeps' rows by
 * layout -- 32 ceil(n/256) ceil(n/512) 512 bytes per system of n bodies).
 * prime: (a, j) of every system at the current x, v, the start levels for macro steps of dt_max_host[s], ticks and
 * counters 0: OVERWRITES acc_*.  d->count must equal offsets[n_systems] (ERR_VALIDATION); a dt_max that is not positive
 * or not finite fails with "Time step must be positive" / "Time step must be a finite number".  Asynchronous.
 * advance: every system to its next macro_steps >= 1 macro boundaries, with the primed G, eps and dt_max, in ONE launch
 * (a fast system does not wait for a slow one at a boundary).  Asynchronous, reads nothing back.  On an unprimed handle,
 * or with another count or pos_x pointer than the primed ones: ERR_STATE.  After one eager advance since the priming it
 * can be recorded into a step graph; before that a recording fails with ERR_STATE.
 * A system whose schedule cannot be (no active body, t not ahead of the current tick or beyond 2^L) writes its own status
 * word and stops; the other systems are unaffected, launches queued behind skip that system only, and the next info
 * fails with ERR_STATE "block-step schedule out of range (system S)" and unprimes the handle.
 * info: system >= 0: that system's counters in the struct above (narrow_launches, wide_launches, narrow_below 0);
 * system == -1: the sums over the systems of block_steps, body_steps, level_steps[], floor_hits and macro_steps, with
 * current_tick 0 (every advance ends at a boundary) and last_n_active 0.  Blocking.
 * state: per-body arrays over ALL bodies of the ensemble, as nbody_hip_hermite_block_state.  Blocking.
 * invalidate, set_precision, set_state_f64 / get_state_f64: as the single-system handle's (the f64 arrays cover all
 * bodies); each of the first three unprimes.
 * Errors: null handle / particle data / arrays: ERR_STATE; data on another device than the context: ERR_VALIDATION. */
typedef struct nbody_hip_hermite_batch nbody_hip_hermite_batch;
NBODY_HIP_API int nbody_hip_hermite_batch_create(nbody_hip_ctx* ctx, size_t max_particles_total, size_t max_systems,
                                                 nbody_hip_hermite_batch** out);
/* Waits for the context's stream, frees the handle.  A runtime that is already gone is answered with OK. */
NBODY_HIP_API int nbody_hip_hermite_batch_destroy(nbody_hip_hermite_batch* h);
NBODY_HIP_API int nbody_hip_hermite_batch_set_params(nbody_hip_hermite_batch* h, float eta, float eta_start,
                                                     int max_level);
NBODY_HIP_API int nbody_hip_hermite_batch_set_precision(nbody_hip_hermite_batch* h, int mode);
NBODY_HIP_API int nbody_hip_hermite_batch_get_precision(nbody_hip_hermite_batch* h, int* mode);
NBODY_HIP_API int nbody_hip_hermite_batch_set_layout(nbody_hip_hermite_batch* h, const size_t* offsets_host,
                                                     size_t n_systems);
NBODY_HIP_API int nbody_hip_hermite_batch_prime(nbody_hip_hermite_batch* h, nbody_particle_data* d, float G, float eps,
                                                const float* dt_max_host);
NBODY_HIP_API int nbody_hip_hermite_batch_invalidate(nbody_hip_hermite_batch* h);
NBODY_HIP_API int nbody_hip_hermite_batch_advance(nbody_hip_hermite_batch* h, nbody_particle_data* d, int macro_steps);
NBODY_HIP_API int nbody_hip_hermite_batch_state(nbody_hip_hermite_batch* h, int* levels, unsigned int* ticks, float* want,
                                                nbody_float4* jerk);
NBODY_HIP_API int nbody_hip_hermite_batch_info(nbody_hip_hermite_batch* h, long long system,
                                               nbody_hip_hermite_block_info_t* out);
NBODY_HIP_API int nbody_hip_hermite_batch_set_state_f64(nbody_hip_hermite_batch* h, nbody_particle_data* d,
                                                        const double* pos_host, const double* vel_host);
NBODY_HIP_API int nbody_hip_hermite_batch_get_state_f64(nbody_hip_hermite_batch* h, nbody_particle_data* d,
                                                        double* pos_host, double* vel_host);

/* ---- ensemble EVENTS: per-system stopping conditions and encounter records (no reference counterpart) ----
 *
 * A scattering experiment is over when its outcome is decided, and the closest approach of a fly-by falls between two
 * call boundaries.  With events configured, each system of an ensemble keeps, ON THE DEVICE and inside the one advance
 * launch, a record of its closest approach and of its first contact, and stops by itself on contact or on a macro-step
 * budget of its own.  Opt-in and additive: a handle on which none of it is configured launches
 * exactly the kernels it launched before; the three calls are declared in nbody_hip_events.h.
 *
 * The model.
 *   - Radii: r[i] >= 0 for every body of the ensemble (default: none, which is all 0).  Budget: limit[s], in macro steps
 *     since the priming; 0 means no limit.
 *   - Seen pairs.  In every block step the seen pairs are the pairs (active target i, source j) of the sweep with
 *     j < n (a padded source never enters), j != i as an index (a coincident pair of two different bodies counts) and a
 *     finite d2.  A pair is seen only from its ACTIVE side: a body that is not corrected in a block step sees nobody in
 *     it (in a close encounter both bodies sit on short steps).  The priming sweep contributes nothing: a system that
 *     starts in contact is caught in its first block step.
 *   - d2 is ONE fp32 value: d2 = fma(dx, dx, fma(dy, dy, dz * dz)), with dx, dy, dz exactly the differences the force
 *     sum uses at the predicted positions (the fp32 difference, or the double-single form in extended precision).
 *   - Keys.  key = bits(d2) << 32 | i << 12 | j with system-local indices (n <= 4,096); bits(d2) order as unsigned
 *     integers because d2 >= 0.  Every reduction is a minimum of these unsigned 64-bit keys, so it depends on no lane,
 *     wave or sub-block order: the order is d2, then i, then j.
 *   - Closest approach (flag TRACK_CLOSEST): the smallest key over all seen pairs of all block steps since the priming,
 *     folded block step by block step with STRICTLY LESS, so the earliest block step wins a tie; recorded with the macro
 *     index and the tick of that block step.
 *   - Contact: a seen pair with rs = r[i] + r[j] (fp32), rs > 0 and d2 < rs * rs.  The FIRST CONTACT is taken from the
 *     first block step that has any pair in contact: the smallest key among that block step's contact pairs, with its
 *     macro index and tick.  It is recorded once and never overwritten until the next priming.
 *   - macro index: the number of macro steps the system had completed since the priming when the block step ran (the
 *     first macro step is 0); tick: the block step's time in (0, 2^max_level] inside that macro step.
 *   - Stopping.  A system with a first contact, when STOP_ON_CONTACT is set, COMPLETES the macro step it is in and then
 *     stops (stopped = 1).  A system stops on the budget when its completed macro steps reach limit[s] (stopped = 2;
 *     contact wins when both hold).  A stopped system is skipped by the rest of the launch and by every later launch of
 *     the event form: none of its memory is touched.  Stopping is not an error: the stop word is separate from the
 *     status word, info keeps working and info(-1) sums what was done.  Up to the stop the system is bit for bit the
 *     unconditioned run and all its bodies are synchronised; the record carries the exact tick.  Stopping AT the contact
 *     tick is not provided; a merger is a pass between two launches (the MERGERS block below).
 *   - prime clears all records and stop words.  set_layout drops the configuration.
 * "None" (n = 1, no contact, closest approach not tracked): d2 = +inf, i = j = 0xFFFFFFFF, macro = 0, tick = 0. */
#define NBODY_HIP_BATCH_EVENTS_TRACK_CLOSEST 1
#define NBODY_HIP_BATCH_EVENTS_STOP_ON_CONTACT 2
typedef struct nbody_hip_batch_event_t {
  unsigned int stopped;                 /* 0 running, 1 contact, 2 budget, 3 escape (ensemble OUTCOMES below),
                                           4 resolved (ensemble HIERARCHIES below) */
  unsigned int reserved;                /* 0 */
  unsigned long long macro_steps_done;  /* completed macro steps since the priming */
  float closest_d2;                     /* the closest approach: d2, the active target i, the source j (system-local) */
  unsigned int closest_i, closest_j;
  unsigned int closest_tick;
  unsigned long long closest_macro;
  float contact_d2;                     /* the first contact */
  unsigned int contact_i, contact_j;
  unsigned int contact_tick;
  unsigned long long contact_macro;
} nbody_hip_batch_event_t;              /* 64 bytes */

/* ---- ensemble OUTCOMES: per-system escape detection and stop-on-escape (no reference counterpart) ----
 *
 * The commonest end of a scattering experiment is that one body leaves, unbound, and never comes back.  With outcomes
 * configured, each system of an ensemble tests for that ON THE DEVICE, at every macro boundary inside the one advance
 * launch, keeps a record of its first escape and, if asked, stops by itself.  Opt-in and
 * additive: a handle on which no outcomes are configured launches exactly the kernels it launched before; the two calls
 * are declared in nbody_hip_outcomes.h.
 *
 * The model.
 *   - Per system s an escape radius r_esc[s] >= 0 (fp32, widened to fp64); 0 means no test for that system.
 *   - The test runs after every COMPLETED macro step of a running system with r_esc[s] > 0 and no first escape yet.  It
 *     uses the state in memory, all bodies synchronised: X = (double)pos + (double)pos_lo and V = (double)vel +
 *     (double)vel_lo as exact fp64 sums (residuals 0 in fp32 mode), m = (double)mass, G = (double)G.  Everything is fp64
 *     with correctly rounded sqrt and /, and no product is fused into a sum (the conventions of the ensemble
 *     diagnostics; csrc/hermite_batch_outcomes_common.h).
 *   - The sums S0 = sum m, S1 = sum m X, S2 = sum m V over the system's n bodies, each term m * X rounded, in this order:
 *     thread t of 512 starts from 0 and adds its bodies t, t + 512, ... in rising order; then, in each wave of 64, lane l
 *     adds lane l + off to itself for off = 32, 16, 8, 4, 2, 1 (lane 0 holds the wave's sum); then the eight waves' sums
 *     are added in rising order, starting from wave 0's.
 *   - For body i with M_r = S0 - m_i > 0 (componentwise, every operation rounded once, sums left to right):
 *       R = (S1 - m_i X_i) / M_r,  U = (S2 - m_i V_i) / M_r     the centre of mass of all the rest, and its velocity
 *       d = X_i - R,  w = V_i - U,  r = sqrt(dx dx + dy dy + dz dz)
 *       dw = dx wx + dy wy + dz wz,  vr = dw / r
 *       e = 0.5 (wx wx + wy wy + wz wz) - (G S0) / r              (unsoftened)
 *     Body i ESCAPES at this boundary when r > r_esc[s] and dw > 0 and e > 0.  Every comparison with a NaN is false.  A
 *     body with M_r <= 0 (or NaN), and the body of a system with n = 1, never escapes.  A massless body can escape.
 *   - The FIRST ESCAPE of a system is taken at the first boundary at which any body escapes: the number of bodies that
 *     escape at that boundary and the lowest escaping index (a sum and a minimum of integers: they depend on no order),
 *     for that body r, vr, e and M_r, and the macro index: the number of macro steps the system has completed since the
 *     priming, so >= 1 (the state at the priming is not examined: a system that starts with an escaper is caught after
 *     its first macro step).  It is recorded once and never overwritten until the next priming.
 *   - Stopping.  With the flag STOP_ON_ESCAPE a system with a first escape stops, stop word 3 in
 *     nbody_hip_batch_event_t.stopped.  At one boundary contact (1) wins over escape (3), which wins over the budget
 *     (2).  Everything said of a stopped system above holds: it is skipped by the rest of the launch and by later
 *     launches, none of its memory is touched, info keeps working.  The test only reads state: up to the stop the system
 *     is bit for bit the unconditioned run.
 *   - prime clears all records and stop words.  set_layout drops the configuration.
 * Limitation.  These are single-body escapers against the centre of mass of ALL the rest.  There is no decomposition into
 * hierarchies: a tight pair that leaves together is judged member by member (its orbital motion about its partner enters
 * e and d.w), and a bound hierarchy wider than r_esc can be misjudged.  Choose r_esc well outside any bound structure of
 * interest.
 * "None" (no escape yet, r_esc = 0, outcomes never configured): escaped = 0, escaper = 0xFFFFFFFF, everything else 0. */
#define NBODY_HIP_BATCH_OUTCOMES_STOP_ON_ESCAPE 1
typedef struct nbody_hip_batch_outcome_t {
  unsigned int escaped;        /* bodies that escape at the boundary of the first escape; 0: none yet */
  unsigned int escaper;        /* the lowest escaping index (system-local); 0xFFFFFFFF: none */
  unsigned long long macro;    /* completed macro steps since the priming at that boundary (>= 1) */
  double r;                    /* the escaper's distance from the centre of mass of the rest */
  double vr;                   /* its radial velocity d.w / r */
  double energy;               /* e above, per unit mass */
  double rest_mass;            /* M_r */
  double reserved;             /* 0 */
  double reserved2;            /* 0: fills the record to 64 bytes, the size of an event record */
} nbody_hip_batch_outcome_t;   /* 64 bytes */

/* ---- ensemble HIERARCHIES: per-system decomposition into nested bound pairs and stop-when-resolved (no reference
 * counterpart) ----
 *
 * The result of a scattering experiment is which body ended up bound to which.  With hierarchies configured, each system
 * of an ensemble is reduced ON THE DEVICE, at every macro boundary inside the one advance launch, to a forest of nested
 * bound pairs; it is recorded as RESOLVED once the forest has fallen into two or more mutually unbound, receding,
 * separated pieces and, if asked, stops by itself.  Opt-in and additive: a handle on which no
 * hierarchies are configured launches exactly the kernels it launched before; the three calls are declared in
 * nbody_hip_hierarchy.h.
 *
 * The model.
 *   - Conventions: those of the outcomes above.  The state in memory at a completed macro boundary, all bodies
 *     synchronised: X = (double)pos + (double)pos_lo and V likewise (residuals 0 in fp32 mode), m = (double)mass,
 *     G = (double)G.  Everything is fp64 with correctly rounded sqrt and /, no product is fused into a sum, sums of three
 *     terms are evaluated left to right, a comparison with a NaN is false (csrc/hermite_batch_hierarchy_common.h).
 *   - Per system s a separation radius r_sep[s] >= 0 (fp32, widened to fp64); 0 means no examination for that system.
 *     Per handle an isolation factor kappa >= 0 (fp32, widened; 0 turns that criterion off) and the flags.
 *   - Only systems with 2 <= n <= NBODY_HIP_BATCH_HIERARCHY_MAX (64) are examined.  A system with n = 1 is never
 *     examined; a system with n > 64 and r_sep[s] > 0 is refused (ERR_VALIDATION).  The ensemble keeps its 4,096 limit.
 *   - Nodes 0 .. n-1 are the bodies, as leaves {m, X, V} with bodies = 1.  The TOP SET starts as all leaves.  Composites
 *     get the ids n, n+1, ... in the order they are made.
 *   - The decomposition is a loop of at most n - 1 rounds.  For every unordered pair p < q (by node id) of the top set:
 *       d = X_q - X_p,  w = V_q - V_p,  M = m_p + m_q
 *       r = sqrt(dx dx + dy dy + dz dz),  v2 = wx wx + wy wy + wz wz
 *       eps = 0.5 v2 - (G M) / r
 *     The pair is a CANDIDATE when M > 0, r > 0 and eps < 0, with a = (G M) / (-2.0 eps).  The candidate with the
 *     smallest a is taken, ties to the smallest p, then the smallest q: a > 0, so this is a minimum of integer keys over
 *     bits(a) and the ids and depends on no lane, wave or thread order.  No candidate: the loop ends.  Otherwise node
 *     c = n + k is made: left = p, right = q, m_c = M, X_c = (m_p X_p + m_q X_q) / M per component (both products
 *     rounded, then the sum, then the quotient), V_c the same way, bodies = bodies_p + bodies_q; it records a, r, eps and
 *       e = sqrt(max(0, 1 + ((2.0 eps) h2) / ((G M)(G M)))),  h = d x w,  h2 = hx hx + hy hy + hz hz.
 *     p and q leave the top set and c joins it.
 *   - RESOLVED.  After the loop K is the size of the top set; apo of a composite top node is a (1 + e), of a leaf 0.
 *     The system is resolved at this boundary when K >= 2 and every pair p < q of top nodes has r > r_sep[s] and
 *     dx wx + dy wy + dz wz > 0 and eps > 0 and r > kappa (apo_p + apo_q).
 *   - Cadence.  The examination runs after every COMPLETED macro step of a running system with r_sep[s] > 0, until the
 *     system is resolved; the state at the priming is not examined.  Each examination overwrites the system's node table
 *     and the running part of its record (macro, K, the node count, the largest top node, the smallest top-pair
 *     separation with its pair).  Once resolved, the record and the table are never overwritten until the next priming:
 *     after a stop they hold the hierarchy at the resolving boundary.
 *   - Stopping.  With the flag STOP_ON_RESOLVED a resolved system stops, stop word 4 in nbody_hip_batch_event_t.stopped.
 *     At one boundary contact (1) wins over escape (3), which wins over resolved (4), which wins over the budget (2).
 *     Everything said of a stopped system above holds: it is skipped by the rest of the launch and by later launches, none
 *     of its memory is touched, info keeps working.  The examination only reads state: up to the stop the system is bit
 *     for bit the unconditioned run.
 *   - prime clears the records, the tables and the stop words.  set_layout drops the configuration.
 * Left out.  No stability judgement of a bound hierarchy: a bound but unstable triple stays one unresolved piece and ends
 * on its budget.  No tidal criterion beyond kappa.  No systems of more than 64 bodies.  No identity across a merger.
 * "None" (never examined, n = 1, r_sep = 0, hierarchies never configured): all 0 but min_sep = +inf and
 * min_p = min_q = 0xFFFFFFFF; every node slot of such a system is zero. */
#define NBODY_HIP_BATCH_HIERARCHY_STOP_ON_RESOLVED 1
#define NBODY_HIP_BATCH_HIERARCHY_MAX 64
typedef struct nbody_hip_batch_hierarchy_t {
  unsigned int resolved;      /* 0 or 1 */
  unsigned int top_count;     /* K */
  unsigned long long macro;   /* completed macro steps at the examined boundary; 0: never examined */
  unsigned int node_count;    /* n + composites made */
  unsigned int largest;       /* bodies in the largest top node */
  double min_sep;             /* smallest r over top pairs; +inf when K < 2 */
  unsigned int min_p, min_q;  /* the pair of min_sep; ties: lowest p, then q */
  double reserved[3];         /* 0 */
} nbody_hip_batch_hierarchy_t; /* 64 bytes */
/* 2 n slots per system, starting at slot 2 offsets[s]; slots at and above node_count are zero */
typedef struct nbody_hip_batch_node_t {
  unsigned int left, right;   /* 0xFFFFFFFF for a leaf */
  unsigned int parent;        /* 0xFFFFFFFF for a top node */
  unsigned int bodies;
  double mass, a, e, r, energy;   /* energy is eps; a = e = r = energy = 0 for a leaf */
  double reserved;            /* 0 */
} nbody_hip_batch_node_t;     /* 64 bytes */

/* ---- ensemble MERGERS: sticky-sphere collisions applied between launches (no reference counterpart) ----
 *
 * A contact (ensemble EVENTS above) can only end an experiment.  With mergers configured, a device pass queued BETWEEN
 * two advance calls merges the recorded contact pair of every system that stopped on contact, shrinks that system by one
 * body in place, primes it again -- that system alone, exactly as prime would a fresh system of the remaining bodies --
 * and lets it run on.  Opt-in, additive and asynchronous: a handle on which no mergers are
 * configured launches exactly the kernels it launched before; the three calls are declared in nbody_hip_mergers.h.
 *
 * The model.
 *   - Which systems merge.  nbody_hip_batch_mergers_apply acts on system s iff its stop word is 1 (contact), its status
 *     word is 0, and its contact record names two different slots i != j, both below the system's live count.  The last
 *     condition is checked on the device: a record that fails it leaves the system stopped and sets the flag
 *     NBODY_HIP_BATCH_MERGER_BAD_RECORD in its merger state.  Every other system is not touched: none of its arrays,
 *     counters or records is written.
 *   - The pair is the recorded FIRST CONTACT, merged unconditionally (sticky spheres) at the boundary the system stopped
 *     at.  Limitation.  The events complete the macro step the contact fell into, so the merger is applied to the
 *     synchronised state at that boundary, not at the contact tick: the pair may have passed through each other or
 *     separated again by then.  Choose dt_max short against the crossing time of a contact.
 *   - Slots.  lo = min(i, j), hi = max(i, j).
 *   - The merged body, all in fp64 from the full state (X = (double)pos + (double)pos_lo, residuals 0 in fp32 mode),
 *     every operation rounded once, no product fused into a sum (csrc/hermite_batch_mergers_common.h); ma, mb the masses
 *     of the slots lo and hi, Xa, Xb, Va, Vb, ra, rb likewise:
 *       M = (double)ma + (double)mb
 *       X = (ma Xa + mb Xb) / M,  V = (ma Va + mb Vb) / M     per component; M == 0: the plain means 0.5 (Xa + Xb)
 *       r = cbrt(ra ra ra + rb rb rb)                         the volume rule
 *     Stored: mass (float)M, pos / vel (float)X / (float)V, in extended state precision the residuals
 *     (float)(X - (double)(float)X), radius (float)r.
 *   - Compaction.  The merged body takes slot lo and keeps that slot's id.  If hi is not the last live slot n - 1, the
 *     body of slot n - 1 moves into hi: position, velocity, mass, the six residuals, radius and id.  Slot n - 1 becomes
 *     dead: mass 0, velocity 0, residuals 0, radius 0, acc 0, id 0xFFFFFFFF, position left as it is.  The device-side live
 *     count of the system becomes n - 1: every kernel of the ensemble reads it, so the system runs on as one of n - 1
 *     bodies.  The layout's offsets keep their meaning as slot ranges; the particle count, info, events and the node
 *     tables are unaffected.  The indices of outcome and hierarchy records are slots; the ids translate.
 *   - ids.  A per-body unsigned int: the system-local index the body had at the priming.  prime resets them to 0 .. n-1
 *     and restores every live count to the layout's n.
 *   - Priming again.  The merged system gets acc, jerk, level, tick = 0 and want exactly as prime computes them for a
 *     system of n - 1 bodies (the same pack, the same sweep over the same tiles in the same order, the same finalize and
 *     start level with eta_start).  Not reset: the step counters, the level counters, the status word, the budget, the
 *     outcome and hierarchy records.
 *   - The event record gets stopped = 0, contact and closest approach "none" (the slots have changed: the tracking starts
 *     over); macro_steps_done is kept.
 *   - The log.  One nbody_hip_batch_merger_t per merger, at most n - 1 per system, in a per-body table: the entries of
 *     system s are [offsets[s], offsets[s] + n_mergers).  The energy deltas are fp64, FROM THE VALUES AS STORED after the
 *     merge, with the primed G and eps in the softened form of the ensemble diagnostics:
 *       delta_ke = 1/2 M |V|^2 - 1/2 ma |Va|^2 - 1/2 mb |Vb|^2
 *       delta_pe = -G (sum over the other live bodies k of (t(merged, k) - t(a, k) - t(b, k))  -  t(a, b)),
 *       t(p, q) = m_p m_q / sqrt(|X_q - X_p|^2 + eps^2)
 *     The sum over k is taken in a fixed order: thread t of 256 starts from 0 and adds its bodies t, t + 256, ...; in each
 *     wave of 64 lane l adds lane l + off for off = 32, 16, 8, 4, 2, 1; then the four waves' sums in rising order.  No
 *     atomics: it is bitwise reproducible.
 *   - One merger per system per pass.  A chain (the merged body overlaps a third) is seen again by the next block step,
 *     stops the system at the next boundary and is merged by the next pass.  Of several contacts inside one macro step
 *     only the recorded first one is merged now.
 *   - A stopped system waits for the end of its launch: there are no mergers inside a launch.
 *   - prime clears the log, the ids and the live counts.  set_layout drops the configuration.
 * Left out.  Stopping or merging at the contact tick; mergers inside a launch; several mergers per system per pass; other
 * radius rules; mass loss; mergers on the single-system handles.
 * A handle that never had mergers configured reports n_live = n, no entries and ids 0 .. n-1. */
#define NBODY_HIP_BATCH_MERGERS_ON 1
#define NBODY_HIP_BATCH_MERGER_BAD_RECORD 1
typedef struct nbody_hip_batch_merger_state_t {
  unsigned int n_live;        /* live bodies: the slots [0, n_live) of the system */
  unsigned int n_mergers;     /* entries of the log since the priming */
  unsigned int flags;         /* NBODY_HIP_BATCH_MERGER_BAD_RECORD */
  unsigned int reserved[5];   /* 0 */
} nbody_hip_batch_merger_state_t; /* 32 bytes */
typedef struct nbody_hip_batch_merger_t {
  unsigned int slot_a, slot_b;       /* lo, hi */
  unsigned int id_a, id_b;           /* their ids before the merger; the merged body keeps id_a */
  unsigned int moved_from;           /* n - 1 when that body moved into slot_b; 0xFFFFFFFF: none */
  unsigned int contact_tick;         /* the contact, copied from the event record */
  unsigned long long contact_macro;
  float contact_d2;
  float radius;                      /* of the merged body */
  double mass;                       /* M in fp64 (the stored mass is (float)M) */
  double delta_ke, delta_pe;
} nbody_hip_batch_merger_t;          /* 64 bytes */

/* ---- ensemble DIAGNOSTICS: per-system fp64 energies, momenta, closest and most bound pairs (no reference counterpart) ----
 *
 * What a user of many small systems asks after every call -- is each system's energy error and momentum to be trusted,
 * which pair is bound with what elements, how close is the closest pair -- answered on the device, in fp64, from the
 * full hi + lo state, in ONE launch with one workgroup per system.  The energy calls above
 * (nbody_hip_*_energy*) stay what they are: fp32 per pair term, from pos_* / vel_* alone.
 *
 * The model.  Take a system of bodies [first, first + n) with 1 <= n <= NBODY_HIP_HERMITE_BLOCK_RESIDENT_MAX (4,096).
 * Its state is:
 *   - X_i = (double)pos_i + (double)pos_lo_i and V_i = (double)vel_i + (double)vel_lo_i.  These are exact fp64 sums.
 *     The residuals are 0 where none are given.
 *   - m_i = (double)mass_i, G = (double)G, eps2 = (double)(eps * eps).  eps2 is the fp32 product, the engine's
 *     convention.
 * Everything below is fp64 arithmetic with correctly rounded sqrt and /.  No fp32 and no rsq approximation appears
 * anywhere.
 *
 * Most bound pair.  Take d = X_j - X_i, w = V_j - V_i, r = |d| (unsoftened) and mu = m_i m_j / (m_i + m_j).
 *   - Over the pairs with r > 0 and m_i + m_j > 0, E_b = 1/2 mu |w|^2 - G m_i m_j / r.
 *   - The pair reported is the argmin of E_b, and only if that minimum is < 0.
 *   - Its elements are a = -G m_i m_j / (2 E_b), h = d x w, epsilon = E_b / mu, and
 *     e = sqrt(max(0, 1 + 2 epsilon |h|^2 / (G (m_i + m_j))^2)).
 *   - These are two-body (Kepler) elements from the UNSOFTENED separation.  With eps > 0 they describe the pair, not the
 *     softened model's energy: `potential` is softened, bind_energy / bind_a / bind_e are not.
 * Ties.  Ties in min_sep and in E_b go to the lexicographically smallest (i, j).
 * Determinism.  Every sum has a fixed order that depends on n alone.  It does not depend on the number of systems, on
 * the system's place in the batch, or on the workgroup.  There are no atomics.  A system's struct is a function of that
 * system's bodies only, and is bitwise reproducible. */
typedef struct nbody_hip_system_diag {
  double mass;          /* sum m_i */
  double com[3];        /* sum m_i X_i / mass; {0,0,0} when mass == 0 */
  double momentum[3];   /* sum m_i V_i */
  double ang_mom[3];    /* sum m_i X_i x V_i, about the origin */
  double kinetic;       /* 1/2 sum m_i |V_i|^2 */
  double potential;     /* -G sum_{i<j} m_i m_j / sqrt(|X_j - X_i|^2 + eps2); a pair with |d|^2 + eps2 == 0 adds nothing */
  double min_sep;       /* min_{i<j} |X_j - X_i| (unsoftened); +inf when n == 1 */
  double bind_energy;   /* E_b of the most bound pair, above; 0 when there is none */
  double bind_a;        /* its semi-major axis  -G m_i m_j / (2 E_b); 0 when there is none */
  double bind_e;        /* its eccentricity; 0 when there is none */
  int min_i, min_j;     /* SYSTEM-LOCAL indices, i < j; -1, -1 when n == 1 */
  int bind_i, bind_j;   /* -1, -1 when no pair has E_b < 0 */
  int n;                /* bodies of the system */
  int status;           /* 0 ok; 1 the offsets of this system are not a legal range (nothing else is written but n = 0) */
} nbody_hip_system_diag;   /* 152 bytes */
/* The generic call, for any particle data (a small Velocity-Verlet run included).  System s is the bodies
 * [offsets[s], offsets[s + 1]); offsets_device is a DEVICE array of n_systems + 1 entries and out_device a device array
 * of n_systems structs.  pos_lo / vel_lo: device rows {lx, ly, lz, 0}, d->count of each, or NULL (residuals 0).
 * Asynchronous on the context's stream; it allocates nothing and reads nothing back, so it can be recorded into a step
 * graph from the first call.  The offsets are checked ON THE DEVICE, per system: one that is not
 * offsets[s] < offsets[s + 1] <= d->count with at most 4,096 bodies gets status = 1, n = 0 and nothing else, no body of
 * it is touched, and the other systems of the call are unaffected.  Only pos_*, vel_* and mass of d are read.
 * Errors: null context, particle data, arrays, offsets or out: ERR_STATE; n_systems == 0 succeeds and does nothing;
 * eps < 0 (or NaN), a count of 0 or above 2^30, more than 2^31 - 1 systems, or data on another device than the
 * context's: ERR_VALIDATION. */
NBODY_HIP_API int nbody_hip_systems_diagnostics(nbody_hip_ctx* ctx, const nbody_particle_data* d,
                                                const nbody_float4* pos_lo_or_null, const nbody_float4* vel_lo_or_null,
                                                const unsigned long long* offsets_device, size_t n_systems, float G,
                                                float eps, nbody_hip_system_diag* out_device);
/* The same structs for the systems of the integrator handles above -- the ensemble handle with its layout, residuals and
 * primed G and eps, the single-system block-step handle with its residuals -- are declared in nbody_hip_diag.h. */

/* ---- measurement helpers -------------------------------------------------- */

/* Runs the direct-force kernel `iters` times back to back on the context's stream between
 * two HIP events and returns the mean milliseconds per launch (blocking).  bench.py's
 * `roofline.achieved` comes from this; rocprofv3's kernel trace must agree. */
NBODY_HIP_API int nbody_hip_time_direct_packed(nbody_hip_ctx* ctx, const nbody_float4* targets,
                                 size_t n_targets, const nbody_float4* sources, size_t n_sources,
                                 nbody_float4* acc_out, float G, float eps2, int iters,
                                 float* ms_per_launch);

/* Direct forces are bitwise reproducible, like the reference's one-thread-per-body loop
 * (ref: force_direct.cu:10-85): in the symmetric (action = -reaction) kernels every contribution to a body
 * goes to a slot of its own and the slots are added in a fixed order.
 *   mode 1 (default)  slot planes when they fit the budget -- 24 GiB AND a quarter of the device memory that is
 *                     free when the workspace has to grow -- otherwise fp64 atomics (their order varies from
 *                     launch to launch: fp32 results differ in the last bit now and then); an allocation
 *                     failure of the slot planes also falls back to the atomic form.  nbody_hip_direct_info
 *                     tells which form a call at a given size takes, and which one the last call took;
 *   mode 2            slot planes REQUIRED: a call that cannot have them fails with NBODY_HIP_ERR_RESOURCE
 *                     instead of switching silently;
 *   mode 0            fp64 atomics; the slot planes the context holds are given back at once.
 * Slot planes: a reaction is one fp32 number per component (12 bytes per body and partner superblock), an
 * I-side sum is fp64 (24 bytes per body and split): 12 D + 24 splits bytes per body with D = N / (512 R) --
 * 1.9 GB at N = 2^20 (round 2: 3.4 GB), ~14 GB at N = 2^22; a workspace more than four times larger than the
 * current call needs is released first.  Time against the atomic form at N = 2^20: see DESIGN.md section 4.1.
 * The one-sided kernel (N < 12,288, rectangular sets) is reproducible anyway; the two-set kernel of the
 * sharded path follows the same switch (splits I-side slots per body of the first set, N_first / (256 R)
 * reaction slots per body of the second). */
NBODY_HIP_API int nbody_hip_direct_deterministic(nbody_hip_ctx* ctx, int mode);

/* Most bytes of slot planes the deterministic form may take on this context (default and bytes = 0: 24 GiB;
 * a quarter of the free device memory is the second limit whatever this says).  For shared GPUs. */
NBODY_HIP_API int nbody_hip_direct_slot_budget(nbody_hip_ctx* ctx, unsigned long long bytes);

/* What a Direct all-pairs call at `count` bodies runs with the context's current settings (plain host
 * arithmetic + one hipMemGetInfo when the workspace would have to grow), and what the last call ran.
 * ctx may be NULL: the answer for a context with default settings from the fixed budget alone (no device needed). */
typedef struct nbody_hip_direct_info_t {
  int deterministic_mode;     /* the context's setting: 0, 1 or 2 (see nbody_hip_direct_deterministic) */
  int kernel;                 /* at `count` bodies: 0 one-sided, 1 symmetric + fp64 atomics, 2 symmetric + slot planes */
  int bodies_per_lane_equal;  /* R of the equal-mass instantiation (symmetric kernels; else 0) */
  int bodies_per_lane_general;/* R of the general-mass instantiation */
  int reaction_slots;         /* D  (equal-mass shape) */
  int iside_slots;            /* splits (equal-mass shape) */
  int reserved0, reserved1;
  unsigned long long workspace_bytes_needed;  /* accumulator workspace of such a call */
  unsigned long long slot_bytes_wanted;       /* what the slot planes need (also when they were refused) */
  unsigned long long workspace_bytes_held;    /* what the context holds right now */
  int last_kernel;            /* what the last Direct call of this context ran (-1: none yet) */
  int reserved2;
} nbody_hip_direct_info_t;
NBODY_HIP_API int nbody_hip_direct_info(nbody_hip_ctx* ctx, size_t count, float eps2, nbody_hip_direct_info_t* out);

/* Tuning knobs for experiments.  variant: -1 automatic, 0 scalar body + LDS sources, 1 packed
 * (v_pk_*_f32) body + LDS sources, 2 scalar body + scalar-cache sources, 3 symmetric (action =
 * -reaction) kernel whenever targets == sources, 4 the same with every fp64 I-side sum in LDS (at 16 bodies per
 * lane: one workgroup per CU instead of two; the same bits, kept for A/B); the others 0 = automatic:
 * targets_per_lane: 1, 2 or 4 (6, 8, 12, 16: symmetric kernel only; 12: all pairs only); source_splits: number of source sub-ranges per target block. */
NBODY_HIP_API int nbody_hip_direct_tuning(nbody_hip_ctx* ctx, int variant, int targets_per_lane,
                            int source_splits);

#ifdef __cplusplus
}
#endif
#endif /* NBODY_HIP_H */
