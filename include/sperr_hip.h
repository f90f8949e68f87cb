/*
 * sperr_hip.h -- C ABI of libsperr_hip.so, the MI355X (gfx950) SPERR 3D chunk-pipeline engine.
 *
 * Two families of entry points:
 *
 * 1. Drop-in replacements for the reference's C API (same names, argument meaning, ownership
 *    and return codes as /root/reference/include/SPERR_C_API.h:106-137,87-92 and
 *    /root/reference/src/SPERR_C_API.cpp:135-258): host buffers in, malloc'd host buffers out.
 *    The per-chunk pipeline (conditioner, CDF 9/7 DWT, quantiser, SPECK3D coder, bit packing)
 *    runs on the GPU(s); `nthreads` (the reference's OpenMP team size, src/SPERR3D_OMP_C.cpp:12-20)
 *    is the number of host threads that stage rows for the transfers.  mode 1 (fixed rate, `quality` = bits per value), mode 2
 *    (fixed PSNR, dB) and mode 3 (fixed point-wise error, the tolerance; the outlier list goes
 *    through the reference's Outlier_Coder / SPECK1D_INT stream format) are implemented.
 *
 * 2. Device-resident entry points (sperrhip_*): the volume and the container stay in HBM, which
 *    is what bench.py times and what an application that already holds its field on the GPU
 *    should call.  All pointers marked `d_` are device pointers; `hip_stream` is a hipStream_t
 *    passed as void* (NULL = the default stream).  A call is ordered on hip_stream: its inputs may
 *    still be pending there (work enqueued on hip_stream before the call writes them), and work
 *    enqueued there after the call returns sees its outputs.  Every call but sperrhip_mask_apply_dev
 *    and sperrhip_mask_expand_dev has also finished when it returns; those two return with their
 *    kernel enqueued (and sperrhip_decompress_masked_dev with its last one, the same store of
 *    `value`).  Concurrent callers pass a stream each; when more call at once than a device
 *    has engines (SPERR_HIP_ENGINES_PER_DEVICE, 4), the others wait on the host.  Many small volumes of one shape that each want a container go
 *    through the batch calls (sperrhip_compress_batch_dev / sperrhip_decompress_batch_dev): one
 *    call for all of them, the same containers as one call per volume.  A box out of each of many
 *    containers -- a region over a time series, crops for a loader -- is one call as well
 *    (sperrhip_decompress_boxes_dev), whatever level or portion it is cut from.
 *
 * There is no CPU fallback: every entry point returns -1 (and prints the HIP error) when no
 * gfx950 device or kernel image is available.
 */
#ifndef SPERR_HIP_H
#define SPERR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- reference-compatible C API (replaces include/SPERR_C_API.h of the reference) ---------- */

/* include/SPERR_C_API.h:106-119 ; returns 0 ok, 1 *dst not NULL, 2 bad parameter, -1 other */
int sperr_comp_3d(const void* src, int is_float, size_t dimx, size_t dimy, size_t dimz,
                  size_t chunk_x, size_t chunk_y, size_t chunk_z, int mode, double quality,
                  size_t nthreads, void** dst, size_t* dst_len);

/* include/SPERR_C_API.h:129-137 */
int sperr_decomp_3d(const void* src, size_t src_len, int output_float, size_t nthreads,
                    size_t* dimx, size_t* dimy, size_t* dimz, void** dst);

/* include/SPERR_C_API.h:87-92 */
void sperr_parse_header(const void* src, size_t* dimx, size_t* dimy, size_t* dimz, int* is_float);

/* include/SPERR_C_API.h:138-156 : keep `pct` percent of every chunk stream (progressive access);
 * the result decodes with sperr_decomp_3d.  Host only: sperrhip_trunc_dev does the same to a container in device
 * memory, and sperrhip_decompress_portion_dev decodes a portion without making one.  Returns 0 ok, 1 *dst not NULL,
 * -1 other. */
int sperr_trunc_3d(const void* src, size_t src_len, unsigned pct, void** dst, size_t* dst_len);

/* ---- chunk farm: the same on an explicit list of devices -----------------------------------
 * sperr_comp_3d / sperr_decomp_3d above run on the chunk farm of sperr_amd/csrc/farm.hip: the
 * volume is cut into work items (runs of equally shaped chunks in chunk_volume order,
 * /root/reference/src/sperr_helper.cpp:542-592), a shared queue hands them to a few worker threads
 * per device, and every worker streams its items through pinned staging buffers (gather -> H2D ->
 * the device pipeline -> D2H), so the volume is never resident on a device as a whole and may be
 * larger than HBM.  This replaces the OpenMP chunk loops of
 * /root/reference/src/SPERR3D_OMP_C.cpp:94-130 and src/SPERR3D_OMP_D.cpp:101-127.
 * They use the devices SPERR_HIP_DEVICES names ("all", the default, or "0,2,3"); the entry points
 * below take the list as an argument (devices == NULL or ndevices == 0: the same default).  An
 * ordinal may repeat.  `nthreads`: host threads that move rows between the caller's buffers and the
 * staging buffers (0 = a default of 4 to 12 per worker, by the host's thread count).  A caller's volume that is pinned host memory
 * (hipHostMalloc / hipHostRegister) is read and written by DMA without staging; a volume that is
 * DEVICE memory (compress: src, decompress: the dst of sperrhip_decomp_3d_into) is handled by the
 * device-resident path on the device it lives on, and only the container crosses the bus.
 * Return codes as sperr_comp_3d / sperr_decomp_3d. */
int sperrhip_comp_3d_farm(const void* src, int is_float, size_t dimx, size_t dimy, size_t dimz,
                          size_t chunk_x, size_t chunk_y, size_t chunk_z, int mode, double quality,
                          size_t nthreads, const int* devices, size_t ndevices, void** dst,
                          size_t* dst_len);
int sperrhip_decomp_3d_farm(const void* src, size_t src_len, int output_float, size_t nthreads,
                            const int* devices, size_t ndevices, size_t* dimx, size_t* dimy,
                            size_t* dimz, void** dst);
/* the volume into a buffer of the caller (dst_bytes of room; it may be pinned memory) */
int sperrhip_decomp_3d_into(const void* src, size_t src_len, int output_float, size_t nthreads,
                            const int* devices, size_t ndevices, void* dst, size_t dst_bytes,
                            size_t* dimx, size_t* dimy, size_t* dimz);
/* Host-only check of the farm's queue (no device is touched): how the chunks of a volume are cut
 * into items and which of ndevices * workers_per_device idle workers takes which.  lockstep != 0:
 * the workers take their items in rounds (all equally fast), which makes the outcome
 * deterministic.  per_worker_chunks[ndevices * workers_per_device], item_of_chunk[nchunks],
 * worker_of_chunk[nchunks] (each may be NULL); worker w belongs to device w mod ndevices. */
int sperrhip_farm_selftest(size_t dimx, size_t dimy, size_t dimz, size_t chunk_x, size_t chunk_y,
                           size_t chunk_z, size_t bytes_per_value, size_t ndevices,
                           size_t workers_per_device, int lockstep, uint32_t* per_worker_chunks,
                           uint32_t* item_of_chunk, uint32_t* worker_of_chunk, size_t* nitems);
/* NUMA placement of the farm.  A worker thread binds itself (its helper threads inherit the mask,
 * the staging memory it pins is first touched by it) to the CPUs of the NUMA node its device hangs
 * off: hipDeviceGetPCIBusId -> <sysfs>/bus/pci/devices/<bdf>/numa_node ->
 * <sysfs>/devices/system/node/node<N>/cpulist.  The reference leaves placement to the OpenMP runtime
 * of its chunk loop (/root/reference/src/SPERR3D_OMP_C.cpp:94-130, SPERR3D_OMP_D.cpp:101-127).
 * SPERR_HIP_FARM_NUMA=0 switches it off, SPERR_HIP_SYSFS_ROOT names another tree.  The first two
 * are host only (no device is touched; sysfs_root NULL = the default tree): what the tree says
 * about a PCI device, and the binding applied to the CALLING thread (returns the number of CPUs it
 * is bound to; 0 = left as it was).  The third reports a device's PCI address, node (-1 unknown)
 * and CPU count as the farm sees them. */
int sperrhip_numa_probe(const char* sysfs_root, const char* pci_bdf, int* node, int* cpus,
                        size_t cpus_cap, size_t* ncpus);
int sperrhip_numa_bind_self(const char* sysfs_root, const char* pci_bdf);
int sperrhip_farm_device_place(int dev, char* bdf, size_t bdf_cap, int* node, size_t* ncpus);
/* Host CPUs this process may use, and what the farm does with them (host only, no device touched).
 * The reference sizes its chunk loop by the caller's nthreads, 0 = omp_get_max_threads()
 * (/root/reference/src/SPERR3D_OMP_C.cpp:12-20).  The farm starts threads of its own, and sizes them by
 * min(affinity mask, cgroup CFS quota) -- cgroup v2 cpu.max, v1 cpu.cfs_quota_us / cpu.cfs_period_us, the
 * tightest over the process's group and its ancestors -- never by the machine's CPU count: a container
 * that shows 256 CPUs and grants 16 throttles what runs beyond 16.  cgroup_root / proc_cgroup NULL = the
 * system's (SPERR_HIP_CGROUP_ROOT / SPERR_HIP_PROC_CGROUP name others).  quota_cpus 0 = unlimited.
 * sperrhip_host_throttle reads cpu.stat (returns 1 when there is none).  sperrhip_farm_threads reports
 * the thread plan for ndevices devices. */
int sperrhip_host_cpus(const char* cgroup_root, const char* proc_cgroup, size_t* visible, size_t* affinity,
                       double* quota_cpus, size_t* usable);
int sperrhip_host_throttle(const char* cgroup_root, const char* proc_cgroup, unsigned long long* nr_throttled,
                           unsigned long long* throttled_usec);
int sperrhip_farm_threads(size_t nthreads, size_t ndevices, size_t* workers_per_device,
                          size_t* dec_workers_per_device, size_t* helpers_per_worker, size_t* threads_total,
                          size_t* cpus_usable);

/* ---- device-resident API ---------------------------------------------------------------------- */

/* Upper bound of the container size sperrhip_compress_dev can produce (bytes). */
size_t sperrhip_max_compressed_size(size_t dimx, size_t dimy, size_t dimz, size_t chunk_x,
                                    size_t chunk_y, size_t chunk_z, int mode, double quality);

/* Compress a volume that lives in device memory (x fastest; float if is_float else double) into
 * a SPERR container written to d_dst (device memory, capacity dst_cap bytes).  *dst_len receives
 * the container length.  Same modes / return codes as sperr_comp_3d (1 is never returned). */
int sperrhip_compress_dev(const void* d_src, int is_float, size_t dimx, size_t dimy, size_t dimz,
                          size_t chunk_x, size_t chunk_y, size_t chunk_z, int mode, double quality,
                          void* d_dst, size_t dst_cap, size_t* dst_len, void* hip_stream);

/* Decompress a container that lives in device memory into d_dst (device memory holding
 * dimx*dimy*dimz floats or doubles; query the dims first with sperrhip_parse_header_dev or keep
 * them from compression).  Returns 0 ok, -1 error. */
int sperrhip_decompress_dev(const void* d_src, size_t src_len, int output_float, void* d_dst,
                            size_t dst_cap_bytes, size_t* dimx, size_t* dimy, size_t* dimz,
                            void* hip_stream);

/* ---- compression to a byte target (the size mode) ------------------------------------------------
 * Fixed-rate mode gives every chunk the same bits per sample, whatever it holds.  These calls give a whole volume a
 * byte target and deal it to the chunks so that all of them stop at (nearly) the same ABSOLUTE threshold q_c 2^p: a
 * chunk of background gets a few bytes, the chunk that holds the feature the rest.  The result is an ordinary
 * fixed-rate container (chunk lengths are in its header): every reader of mode-1 containers opens it.
 *
 * sperrhip_chunk_count: the chunks the container of such a volume has (0: a dimension is 0) -- the entries the calls
 * below write into the caller's host arrays.  nchunks_cap / budgets_cap state how many entries those arrays hold: a
 * call whose arrays are too short returns -1 and writes nothing.
 *
 * sperrhip_size_survey_dev: what any threshold would cost, without compressing.  Per chunk, in container order (host
 * arrays of nchunks entries): q[c] the fixed-rate quantisation step, nbp[c] the number of bit planes, end[c * 32 + p]
 * the chunk stream's payload bits at the end of plane p under an unlimited budget (zeros from nbp[c] on), is_const[c]
 * whether the chunk is constant (17 bytes, no planes).  Coding chunk c down to plane p leaves an error of the order
 * of q[c] 2^p and takes 26 + end[c * 32 + p] / 8 bytes.
 *
 * sperrhip_compress_size_dev: a container of at most target_bytes bytes.  budgets (host, nchunks entries, may be NULL)
 * receives every chunk's budget in bits: a multiple of 8, 0 for a constant chunk.  The container is shorter than the
 * target by less than nchunks + 1 bytes, or by more when the target is beyond every chunk's 32 planes coded in full
 * (this call never widens the coefficients to 64 bits).  Returns 0 ok; -1, with nothing written to d_dst, when the
 * target does not hold the headers and one payload byte per chunk that is not constant.
 * Volumes as sperrhip_compress_dev takes them in mode 1; no views, batches, fields, masked or relative volumes. */
size_t sperrhip_chunk_count(size_t dimx, size_t dimy, size_t dimz, size_t chunk_x, size_t chunk_y, size_t chunk_z);
int sperrhip_size_survey_dev(const void* d_src, int is_float, size_t dimx, size_t dimy, size_t dimz, size_t chunk_x,
                             size_t chunk_y, size_t chunk_z, size_t nchunks_cap, double* q, int32_t* nbp, uint64_t* end,
                             uint8_t* is_const, void* hip_stream);
int sperrhip_compress_size_dev(const void* d_src, int is_float, size_t dimx, size_t dimy, size_t dimz, size_t chunk_x,
                               size_t chunk_y, size_t chunk_z, size_t target_bytes, void* d_dst, size_t dst_cap,
                               size_t* dst_len, uint64_t* budgets, size_t budgets_cap, void* hip_stream);

/* Reads the container header of a device-resident container on the default stream, which does not wait for a
 * non-blocking stream: for a container that work on another stream is still writing, use the _stream_ call.
 * Returns 0 ok. */
int sperrhip_parse_header_dev(const void* d_src, size_t src_len, size_t* dimx, size_t* dimy,
                              size_t* dimz, int* is_float, size_t* chunk_x, size_t* chunk_y,
                              size_t* chunk_z);
/* The same on hip_stream: the header is read behind everything enqueued there (NULL: the call above). */
int sperrhip_parse_header_stream_dev(const void* d_src, size_t src_len, size_t* dimx, size_t* dimy,
                                     size_t* dimz, int* is_float, size_t* chunk_x, size_t* chunk_y,
                                     size_t* chunk_z, void* hip_stream);

/* ---- stage access for parity tests (device pointers; one chunk = the whole array) ------------- */

/* In-place forward / inverse CDF 9/7 3D transform of dimx*dimy*dimz doubles. */
int sperrhip_dwt3d_dev(double* d_vals, size_t dimx, size_t dimy, size_t dimz, int inverse,
                       void* hip_stream);

/* SPECK3D-encode one chunk of already quantised coefficients.  width is 4 or 8 (bytes per
 * magnitude); d_sign holds (n+63)/64 words, bit i set = non-negative.  budget_bits 0 = unlimited.
 * The 9-byte-header stream is written to d_dst; *dst_len receives its length.
 * dimz = 0 means a dimx x dimy slice through the 2D coder (SPECK2D_INT: the quadtree forest and the type-I set), with
 * n = dimx * dimy coefficients; dimz = 1 is a one-sample-thick chunk of the 3D coder, whose stream differs. */
int sperrhip_speck3d_encode_dev(const void* d_coef, int width, const uint64_t* d_sign, size_t dimx,
                                size_t dimy, size_t dimz, size_t budget_bits, void* d_dst,
                                size_t dst_cap, size_t* dst_len, void* hip_stream);

/* The plane table of one chunk of quantised coefficients, as given to sperrhip_speck3d_encode_dev: end[p], p < 64 (host
 * memory), receives the stream's length in bits at the end of bit plane p -- after its sorting and its refinement pass --
 * under an unlimited budget, zeros from the plane count *nbp on.  It is counted from the set pyramid and the pixel
 * census; no stream is written.  width must be 4; the 64-bit coefficient pass and 2D slices (dimz = 0) are refused
 * with -1. */
int sperrhip_speck3d_plane_bits_dev(const void* d_coef, int width, const uint64_t* d_sign, size_t dimx, size_t dimy,
                                    size_t dimz, uint64_t* end, int* nbp, void* hip_stream);

/* The outlier coder of point-wise error mode (mode 3) on its own: d_orig (floats when is_float,
 * else doubles) and d_recon (doubles) hold nchunks chunks of dimx*dimy*dimz samples stacked along
 * z; every sample whose error d_orig - d_recon is beyond tol is an outlier, and chunk c's outlier
 * stream -- what follows its SPECK stream in a container -- is written to d_dst behind chunk
 * c - 1's; lens[c] (host memory) receives its length, 0 for a chunk without outliers.  It runs the
 * stage sperrhip_compress_dev runs behind its own reconstruction, with a mean of 0 and no constant
 * chunk.  Returns 0 ok, 2 for bad arguments, -1 otherwise: an output that is too small, or an
 * error of 2^63 and more, which the reference refuses (src/Outlier_Coder.cpp:88-91). */
int sperrhip_outlier_encode_dev(const void* d_orig, int is_float, const double* d_recon,
                                size_t dimx, size_t dimy, size_t dimz, size_t nchunks, double tol,
                                void* d_dst, size_t dst_cap, size_t* lens, void* hip_stream);

/* Inverse of sperrhip_speck3d_encode_dev: d_coef (width 4 if the header says <= 32 planes, else 8) and d_sign are
 * outputs. *width_out receives the width that was written.  dimz = 0, as there: the stream of a dimx x dimy slice. */
int sperrhip_speck3d_decode_dev(const void* d_stream, size_t stream_len, size_t dimx, size_t dimy,
                                size_t dimz, void* d_coef, uint64_t* d_sign, int* width_out,
                                void* hip_stream);

/* ---- 2D slices -------------------------------------------------------------------------------
 * Drop-in replacements for /root/reference/include/SPERR_C_API.h:53-81
 * (src/SPERR_C_API.cpp:7-134): one slice through SPECK2D_FLT (dwt2d, SPECK2D_INT), the three
 * modes of sperr_comp_3d; out_inc_header != 0 prepends the 10-byte header {version, flags,
 * u32 dimx, u32 dimy}; sperr_decomp_2d takes the stream WITHOUT that header. */
int sperr_comp_2d(const void* src, int is_float, size_t dimx, size_t dimy, int mode, double quality,
                  int out_inc_header, void** dst, size_t* dst_len);
int sperr_decomp_2d(const void* src, size_t src_len, int output_float, size_t dimx, size_t dimy,
                    void** dst);
/* the same on device-resident buffers */
size_t sperrhip_max_compressed_size_2d(size_t dimx, size_t dimy, int mode, double quality);
int sperrhip_compress_2d_dev(const void* d_src, int is_float, size_t dimx, size_t dimy, int mode,
                             double quality, int out_inc_header, void* d_dst, size_t dst_cap,
                             size_t* dst_len, void* hip_stream);
int sperrhip_decompress_2d_dev(const void* d_src, size_t src_len, int output_float, size_t dimx,
                               size_t dimy, void* d_dst, size_t dst_cap_bytes, void* hip_stream);

/* ---- multi-resolution decoding ---------------------------------------------------------------
 * sperr::SPERR3D_OMP_D::decompress(p, multi_res = true) + release_hierarchy()
 * (/root/reference/include/SPERR3D_OMP_D.h:22-29, src/SPERR3D_OMP_D.cpp:50-150,
 * src/CDF97.cpp:150-168, src/SPECK_FLT.cpp:592-603): besides the volume, the volume at every
 * coarsened resolution of the chunks (src/sperr_helper.cpp:70-123), coarsest first, as doubles.
 * Exists only when the chunks are dyadic and tile the volume; otherwise there are 0 levels. */
/* number of levels and their dims (level_dims: 3 entries per level, x y z; room for 16 levels) */
int sperrhip_multires_levels(size_t dimx, size_t dimy, size_t dimz, size_t chunk_x, size_t chunk_y,
                             size_t chunk_z, size_t* nlev, size_t* level_dims);
/* d_levels: host array of `nlev` device pointers, level h sized by sperrhip_multires_levels */
int sperrhip_decompress_multires_dev(const void* d_src, size_t src_len, int output_float,
                                     void* d_dst, size_t dst_cap_bytes, size_t nlev,
                                     double* const* d_levels, void* hip_stream);
/* host buffers: *dst must be NULL; *dst and levels[0 .. *nlev) are malloc'd (free() them) */
int sperrhip_decomp_3d_multires(const void* src, size_t src_len, int output_float, size_t* dimx,
                                size_t* dimy, size_t* dimz, void** dst, size_t* nlev,
                                size_t* level_dims, double** levels);

/* The same for a slice: SPECK2D_FLT::decompress(multi_res = true) + release_hierarchy()
 * (/root/reference/src/SPECK2D_FLT.cpp:52-58, src/CDF97.cpp:114-130,566-579,
 * src/SPECK_FLT.cpp:592-603; what utilities/sperr2d.cpp --decomp_lowres_f/_d writes): the slice at
 * every coarsened resolution (src/sperr_helper.cpp:86-95), coarsest first, as doubles.  Every
 * slice shape has them (none if the shorter side is below 8).  level_dims: 2 entries per level
 * (x y), room for 16 levels.  `src` is the stream WITHOUT the 10-byte header, as for
 * sperr_decomp_2d. */
int sperrhip_multires_levels_2d(size_t dimx, size_t dimy, size_t* nlev, size_t* level_dims);
int sperrhip_decompress_2d_multires_dev(const void* d_src, size_t src_len, int output_float,
                                        size_t dimx, size_t dimy, void* d_dst, size_t dst_cap_bytes,
                                        size_t nlev, double* const* d_levels, void* hip_stream);
/* host buffers: *dst must be NULL; *dst and levels[0 .. *nlev) are malloc'd (free() them) */
int sperrhip_decomp_2d_multires(const void* src, size_t src_len, int output_float, size_t dimx,
                                size_t dimy, void** dst, size_t* nlev, size_t* level_dims,
                                double** levels);

/* ---- a sub-box of a 3D container ------------------------------------------------------------- */
/* The box [lo, lo + dims) of the volume, decoded from the chunks it meets only: no byte of any other
 * chunk's stream is read.  The result is the box cut out of the whole decode, bit for bit, as
 * box_dims[0]*box_dims[1]*box_dims[2] values, x fastest.  Any container kind decodes this way
 * (fixed-rate, PSNR, point-wise error, truncated; fp32 or fp64 data, float or double output).  The
 * calls return -1 without writing to the output when an extent is 0, when lo + dims leaves the
 * volume, when the output is too small, or when the container is refused as
 * sperrhip_decompress_dev refuses it. */
/* host only: the ids (chunk_volume order) of the chunks the box meets.  Returns 0 ok (*count ids
 * written), 1 when `ids` is NULL or `cap` is less than *count (nothing written), -1 bad box. */
int sperrhip_box_chunks(size_t dimx, size_t dimy, size_t dimz, size_t chunk_x, size_t chunk_y,
                        size_t chunk_z, const size_t box_lo[3], const size_t box_dims[3],
                        uint32_t* ids, size_t cap, size_t* count);
/* device container -> device box on `hip_stream` (its device). Returns 0 ok, -1 error. */
int sperrhip_decompress_box_dev(const void* d_src, size_t src_len, int output_float,
                                const size_t box_lo[3], const size_t box_dims[3], void* d_dst,
                                size_t dst_cap_bytes, void* hip_stream);
/* host container -> malloc'd host box (*dst must be NULL, free() it).  The chosen chunks' bytes
 * travel to the calling thread's device, packed; one device does the work.  Returns 0 ok,
 * 1 *dst not NULL, -1 error. */
int sperrhip_decomp_3d_box(const void* src, size_t src_len, int output_float,
                           const size_t box_lo[3], const size_t box_dims[3], void** dst);

/* ---- one level of a 3D container's hierarchy, whole or a box of it ---------------------------- */
/* Level `level` of the hierarchy (0 <= level < nlev, coarsest first as sperrhip_multires_levels orders
 * them), or the box [lo, lo + dims) of it given in that level's coordinates: bit for bit that level of
 * sperrhip_decompress_multires_dev cut to the box, as doubles, or as floats each narrowed once (round
 * to nearest).  Only the chunks the box meets are read, only the inverse passes of the levels coarser
 * than `level` run, and no outlier stream is looked at (a level is taken before the correctors are
 * added); nothing of the full volume's size is allocated.  Any container kind that has levels decodes
 * this way.  The calls return -1 without writing to the output when the container has no such level
 * (chunks that are not dyadic or do not tile the volume have none), when an extent is 0, when
 * lo + dims leaves the level, when only one of box_lo / box_dims is NULL, when the output is too
 * small, or when the container is refused as sperrhip_decompress_dev refuses it. */
/* box_lo and box_dims both NULL: the whole level.  Output: box_dims (or the level's dims) values, x fastest. */
int sperrhip_decompress_level_dev(const void* d_src, size_t src_len, int output_float, size_t level,
                                  const size_t box_lo[3], const size_t box_dims[3], void* d_dst,
                                  size_t dst_cap_bytes, void* hip_stream);   /* 0 ok, -1 */
/* host container -> malloc'd host level or box (*dst must be NULL, free() it); out_dims receives its
 * dims.  The chosen chunks' bytes travel to the calling thread's device, packed.  Returns 0 ok,
 * 1 *dst not NULL, -1 error. */
int sperrhip_decomp_3d_level(const void* src, size_t src_len, int output_float, size_t level,
                             const size_t box_lo[3], const size_t box_dims[3], size_t out_dims[3],
                             void** dst);

/* ---- a portion of a 3D container: decoding at a fraction of the bit rate, truncating on the device -- */
/* SPERR streams are embedded: the first `pct` percent of every chunk's stream decode to a coarser version of the
 * same field (the reference's src/SPERR3D_Stream_Tools.cpp:134-226, utilities/sperr3d_trunc.cpp).  How many bytes
 * of a chunk stream of chunk_len bytes a portion keeps: all of them when pct is 0 or >= 100 or chunk_len <= 64,
 * else max(64, floor(pct / 100 * chunk_len)) (SPERR3D_Stream_Tools.cpp:170-195).  Host only. */
size_t sperrhip_portion_len(size_t chunk_len, unsigned pct);
/* The volume (level == NULL, no box), the box [lo, lo + dims) of it (level == NULL), or level *level of the hierarchy
 * whole or a box of it (box_lo and box_dims NULL or not as for sperrhip_decompress_level_dev), decoded from the first
 * `pct` percent of every chunk stream: bit for bit what sperrhip_decompress_dev / _box_dev / _level_dev give for
 * sperr_trunc_3d(container, pct), but no truncated container is made -- no byte behind a kept prefix is read and the
 * decoder's workspace follows the kept lengths.  pct 0 or >= 100: the whole streams, exactly as those calls.  They
 * return -1 without writing to the output where those calls do, and when only one of box_lo / box_dims is NULL. */
int sperrhip_decompress_portion_dev(const void* d_src, size_t src_len, unsigned pct, int output_float,
                                    const size_t* level, const size_t box_lo[3], const size_t box_dims[3],
                                    void* d_dst, size_t dst_cap_bytes, void* hip_stream);      /* 0 ok, -1 */
/* host container -> malloc'd host volume, box or level (*dst must be NULL, free() it); out_dims (may be NULL) receives
 * its dims.  Only the kept prefixes of the chosen chunks travel to the calling thread's device, one copy per chunk.
 * Returns 0 ok, 1 *dst not NULL, -1 error. */
int sperrhip_decomp_3d_portion(const void* src, size_t src_len, unsigned pct, int output_float,
                               const size_t* level, const size_t box_lo[3], const size_t box_dims[3],
                               size_t out_dims[3], void** dst);
/* sperr_trunc_3d of a container in device memory into device memory: d_dst receives byte for byte what
 * sperr_trunc_3d makes of it, *dst_len its length.  One kernel launch moves all bytes; the ranges may have any
 * alignment.  Returns 0 ok; 1 when d_dst is NULL or dst_cap is too small -- nothing is written and *dst_len holds the
 * size needed (src_len always suffices); -1 for a NULL d_src or dst_len, a container sperrhip_decompress_dev would
 * refuse, or source and destination ranges that overlap. */
int sperrhip_trunc_dev(const void* d_src, size_t src_len, unsigned pct, void* d_dst, size_t dst_cap,
                       size_t* dst_len, void* hip_stream);
/* nvol containers, container v at [offsets[v], offsets[v+1]) of d_src (host array), each truncated as above and
 * written back to back: container v of the result is [out_offsets[v], out_offsets[v+1]) of d_dst (host array of
 * nvol + 1 entries; out_offsets[nvol] is the size needed when 1 is returned).  The containers need not describe the
 * same volume.  Return codes as sperrhip_trunc_dev; -1 also for nvol == 0 and decreasing offsets. */
int sperrhip_trunc_batch_dev(const void* d_src, const size_t* offsets, size_t nvol, unsigned pct,
                             void* d_dst, size_t dst_cap, size_t* out_offsets, void* hip_stream);

/* ---- quality figures of a reconstruction, both arrays in device memory ------------------------- */
/* out[8] = {rmse, linfty, psnr, min, max, mean, var, mse}: calc_stats<T> then calc_mean_var<T> of the
 * reference (min, max, mean and var are the original's), each a T widened to double, with the reference's
 * blocked, strictly sequential sums in T -- the bits a host run of the reference gives; psnr goes through
 * the host's log10.  Identical arrays: rmse 0, linfty 0, psnr +inf, mse 0.  The arrays hold n values of
 * float (is_float != 0) or double at any alignment of that type; values are finite (NaNs are the caller's
 * problem, as in the reference) and the sign of a zero min or max is not pinned.  One host wait, at the
 * end.  0 ok; -1 (out untouched, nothing launched) for n == 0 or a NULL pointer. */
int sperrhip_quality_dev(const void* d_orig, const void* d_recon, int is_float, size_t n,
                         double* out, void* hip_stream);
/* nvol arrays of n values back to back in each buffer; out[nvol*8]; volume v's figures are bit for
 * bit those of the single call on its slice.  One host wait for the batch; -1 also for nvol == 0. */
int sperrhip_quality_batch_dev(const void* d_orig, const void* d_recon, int is_float, size_t nvol,
                               size_t n, double* out, void* hip_stream);

/* ---- strided views of device arrays -------------------------------------------------------------
 * The interior of an array with ghost cells, a slice of a larger tensor: a volume of dims (dimx, dimy, dimz), x
 * fastest with unit x stride, given by the device address of its first element and two pitches in elements --
 * pitch_y from one row to the next, pitch_z from one slice to the next.  A view is valid when pitch_y >= dimx,
 * pitch_z >= pitch_y * dimy, pitch_z is a multiple of pitch_y and nothing overflows size_t; it reaches
 * (dimz-1)*pitch_z + (dimy-1)*pitch_y + dimx elements from its first one, its extent.  The first element needs the
 * alignment of its type only.  The dense volume is the view {dimx, dimx*dimy}.  No packed copy is made anywhere.
 * The three calls return -1 before anything is written for a view that is not valid, for a NULL pointer, and for an
 * output whose capacity -- in bytes, counted from the view's first element -- is below the view's extent. */
typedef struct sperrhip_view {
  size_t pitch_y, pitch_z;
} sperrhip_view;
/* sperrhip_compress_dev of the view `view` of d_src (its first element): the container is byte for byte the one
 * sperrhip_compress_dev makes of the packed copy.  Same modes and return codes. */
int sperrhip_compress_view_dev(const void* d_src, const sperrhip_view* view, int is_float, size_t dimx, size_t dimy,
                               size_t dimz, size_t chunk_x, size_t chunk_y, size_t chunk_z, int mode, double quality,
                               void* d_dst, size_t dst_cap, size_t* dst_len, void* hip_stream);
/* The volume of a container (box_lo and box_dims NULL) or the box [lo, lo + dims) of it, from the first `pct` percent
 * of every chunk stream (0 or >= 100: all of them), into the view `view` of d_dst whose dims are the volume's or the
 * box's: bit for bit what sperrhip_decompress_dev / _box_dev / _portion_dev write densely.  Elements of the
 * destination that lie outside the view are not written.  dst_cap_bytes counts from d_dst.  0 ok, -1 error (also
 * when only one of box_lo / box_dims is NULL). */
int sperrhip_decompress_view_dev(const void* d_src, size_t src_len, unsigned pct, int output_float,
                                 const size_t box_lo[3], const size_t box_dims[3], void* d_dst,
                                 const sperrhip_view* view, size_t dst_cap_bytes, void* hip_stream);
/* sperrhip_quality_dev of two arrays of dims (dimx, dimy, dimz) read through views; either view may be NULL, which
 * means dense, and the two may differ.  out[8] is bit for bit what sperrhip_quality_dev gives for the two packed
 * copies.  Three kernels, one copy and one host wait, as there.  dimx and dimy stay below 2^31. */
int sperrhip_quality_view_dev(const void* d_orig, const sperrhip_view* view_orig, const void* d_recon,
                              const sperrhip_view* view_recon, int is_float, size_t dimx, size_t dimy, size_t dimz,
                              double* out, void* hip_stream);

/* ---- compression to a PSNR of the whole volume -----------------------------------------------------
 * Mode 2 is the reference's rule chunk by chunk: every chunk is coded to `psnr` dB of the range of its OWN samples, so a
 * chunk of still air beside the plume is coded to 80 dB of its own tiny range.  These calls take the range once, of
 * the whole volume or from the caller, and give every chunk the same target error
 *   t = (range * range) * pow(10, -psnr / 10),
 * from which each chunk's quantisation step is the reference's own search started at q_0 = 2 sqrt(3 t): the first of
 * q_k = q_0 / 2^(k/4), k = 0 .. 4, whose estimated error is at most t (five rungs are all a mid-tread quantiser can
 * need).  The result is an ordinary container -- its header records no mode --, and every chunk stream in it is the
 * reference's for that chunk at that q.  As in mode 2 the target is the reference's estimate, not a guarantee.
 *
 * sperrhip_psnr_ladder: t and the five q of a range (positive, finite) and a target (finite), host libm in the
 * reference's order of operations; -1 when they give no positive finite step.  Host only.
 *
 * sperrhip_range_dev: the smallest and the largest sample of a volume, dense (view NULL) or a view; one streaming read
 * and one wait of the host.  -1 (vmin, vmax untouched) for a NULL pointer, an empty or invalid view, and when a sample
 * is a NaN; an infinity is an extreme like any other.
 *
 * sperrhip_compress_psnr_dev: the container.  range 0 means the volume's own, double(max) - double(min); a positive one
 * is taken as it is (a time series' common range, a range known from the simulation).  dst_cap as
 * sperrhip_max_compressed_size(..., 2, psnr) says.  Returns -1 before anything is launched for a NULL pointer, an
 * invalid view, a zero dimension, a psnr that is not finite, a range that is negative or not finite; -1 with *dst_len
 * and d_dst untouched for a volume whose own range is not finite (a NaN or an infinity among the samples, also when a
 * range is given) and when a chunk's largest coefficient is 2^63 steps or more.  A constant volume gives the container
 * of constant chunks.  One volume; no batches, fields, masked or relative volumes, no 2D slices. */
int sperrhip_psnr_ladder(double range, double psnr, double* t, double* q /* [5] */);
int sperrhip_range_dev(const void* d_src, const sperrhip_view* view /* NULL: dense */, int is_float, size_t dimx,
                       size_t dimy, size_t dimz, double* vmin, double* vmax, void* hip_stream);
int sperrhip_compress_psnr_dev(const void* d_src, const sperrhip_view* view /* NULL: dense */, int is_float, size_t dimx,
                               size_t dimy, size_t dimz, size_t chunk_x, size_t chunk_y, size_t chunk_z, double psnr,
                               double range /* 0: the volume's own */, void* d_dst, size_t dst_cap, size_t* dst_len,
                               void* hip_stream);

/* ---- interleaved fields of a device array ---------------------------------------------------------
 * An array that keeps several variables per sample, the variables innermost -- a solver's (z, y, x, nvar), a detector's
 * (y, x, channel), a channels-last tensor -- compressed to and decoded from one container per field without a packed
 * copy of the caller's making.  The layout is three numbers in elements: stride_x from one sample to the next along x
 * (the record's width), pitch_y from row to row, pitch_z from slice to slice.  A call names nfields consecutive fields;
 * its data pointer is the device address of the FIRST SELECTED field at (0, 0, 0), and field f of sample (x, y, z)
 * lies z*pitch_z + y*pitch_y + x*stride_x + f elements from it.  A layout is valid when the dims are not empty,
 * 1 <= nfields <= stride_x, pitch_y >= dimx*stride_x, pitch_z >= pitch_y*dimy (pitch_z need not be a multiple of
 * pitch_y) and nothing overflows size_t; it reaches (dimz-1)*pitch_z + (dimy-1)*pitch_y + (dimx-1)*stride_x + nfields
 * elements, its extent.  A NULL layout means the dense interleave {nfields, dimx*nfields, dimx*dimy*nfields}.  The
 * first element needs the alignment of its type only.  As in the batch calls nfields * dimz <= 2^32 - 1; dimx, dimy
 * and stride_x stay below 2^31.
 * The calls stage: one kernel gathers the selected fields into stacked volumes in a buffer the library owns (it grows
 * on demand and goes back with sperrhip_release), or scatters them from it, and the batch code runs on that buffer.
 * Every call returns -1 before anything is launched or written for a layout that is not valid or a NULL pointer. */
typedef struct sperrhip_fields {
  size_t stride_x, pitch_y, pitch_z;
} sperrhip_fields;
/* nfields containers back to back in d_dst, container f at [offsets[f], offsets[f + 1]) (offsets: nfields + 1
 * entries): byte for byte what sperrhip_compress_dev makes of the packed copy of field f.  All modes, both
 * precisions; dst_cap at least sperrhip_max_compressed_size_batch(nfields, ...); the return codes of
 * sperrhip_compress_batch_dev. */
int sperrhip_compress_fields_dev(const void* d_src, const sperrhip_fields* layout, size_t nfields, int is_float,
                                 size_t dimx, size_t dimy, size_t dimz, size_t chunk_x, size_t chunk_y, size_t chunk_z,
                                 int mode, double quality, void* d_dst, size_t dst_cap, size_t* offsets,
                                 void* hip_stream);
/* nfields containers (as sperrhip_decompress_batch_dev takes them: any mode, rate, truncation, chunking and coded
 * precision each) whose dims all equal (dimx, dimy, dimz), decoded into the nfields fields of d_dst that `layout`
 * names: field f holds bit for bit what sperrhip_decompress_dev makes of container f.  Only selected fields of samples
 * inside the dims are written; other fields, paddings and halos keep their bytes.  dst_cap_bytes counts from d_dst and
 * must hold the extent.  The decode goes to the library's buffer first, so after ANY refusal or decoder error -- a
 * damaged stream found mid-decode included -- d_dst is as it was.  0 ok, -1 error. */
int sperrhip_decompress_fields_dev(const void* d_src, const size_t* offsets, size_t nfields, int output_float,
                                   size_t dimx, size_t dimy, size_t dimz, void* d_dst, const sperrhip_fields* layout,
                                   size_t dst_cap_bytes, void* hip_stream);
/* out[8 * nfields]: field f's eight figures are bit for bit sperrhip_quality_dev of the packed copies of field f of
 * the two arrays, which may have different layouts. */
int sperrhip_quality_fields_dev(const void* d_orig, const sperrhip_fields* layout_orig, const void* d_recon,
                                const sperrhip_fields* layout_recon, size_t nfields, int is_float, size_t dimx,
                                size_t dimy, size_t dimz, double* out, void* hip_stream);
/* Stage access: the two kernels alone, between an interleaved array and the caller's own stacked buffer (nfields
 * dense volumes back to back, what the batch calls take and return).  The gather's d_dst holds nfields*dimx*dimy*dimz
 * elements within dst_cap_bytes; the scatter's d_dst holds the layout's extent within dst_cap_bytes and is written
 * only at selected fields.  Both wait for the stream.  0 ok, -1 error. */
int sperrhip_fields_gather_dev(const void* d_src, const sperrhip_fields* layout, size_t nfields, int is_float,
                               size_t dimx, size_t dimy, size_t dimz, void* d_dst, size_t dst_cap_bytes,
                               void* hip_stream);
int sperrhip_fields_scatter_dev(const void* d_src, size_t nfields, int is_float, size_t dimx, size_t dimy, size_t dimz,
                                void* d_dst, const sperrhip_fields* layout, size_t dst_cap_bytes, void* hip_stream);

/* ---- a batch of same-shape volumes, one container each ----------------------------------------- */
/* N volumes of the same dims in one call: the chunks of every volume are coded together (a batch is
 * more chunks for the same shape groups), and each volume gets a container of its own.  Container v
 * is byte for byte what sperrhip_compress_dev makes of volume v alone, and volume v of a batch decode
 * is bit for bit sperrhip_decompress_dev of container v.  Chunk origins of the batch, read as one
 * volume of dims (x, y, nvol * z), are 32-bit: nvol * dimz and the batch's chunk count must not
 * exceed 2^32 - 1.  The batch calls return -1 for nvol == 0, a zero dim, a NULL pointer, an output
 * that is too small, decreasing offsets, a container sperrhip_decompress_dev would refuse, or
 * containers whose volume dims differ; a refusal found before decoding starts leaves d_dst as it
 * was, and compression never writes past dst_cap. */
/* Upper bound for sperrhip_compress_batch_dev: nvol times the single-volume bound; 0 if that overflows size_t. */
size_t sperrhip_max_compressed_size_batch(size_t nvol, size_t dimx, size_t dimy, size_t dimz, size_t chunk_x,
                                          size_t chunk_y, size_t chunk_z, int mode, double quality);
/* nvol volumes back to back in d_src; volume v starts at element v*dimx*dimy*dimz, x fastest.
 * Writes nvol containers back to back into d_dst.  offsets (host, nvol + 1 entries) receives the byte ranges:
 * container v is [offsets[v], offsets[v+1]).  Return codes as sperrhip_compress_dev. */
int sperrhip_compress_batch_dev(const void* d_src, int is_float, size_t nvol, size_t dimx, size_t dimy, size_t dimz,
                                size_t chunk_x, size_t chunk_y, size_t chunk_z, int mode, double quality,
                                void* d_dst, size_t dst_cap, size_t* offsets, void* hip_stream);
/* nvol containers back to back in d_src, container v at [offsets[v], offsets[v+1]) (host array).  All of them
 * must describe the same volume dims.  Chunk dims, mode, rate, truncation and is_float may differ.  d_dst receives
 * nvol volumes back to back (float or double).  *dimx..*dimz receive the shared dims.  Returns 0 ok, -1 error. */
int sperrhip_decompress_batch_dev(const void* d_src, const size_t* offsets, size_t nvol, int output_float,
                                  void* d_dst, size_t dst_cap_bytes, size_t* dimx, size_t* dimy, size_t* dimz,
                                  void* hip_stream);

/* ---- a box per entry out of a batch of containers --------------------------------------------- */
/* The same region of N time steps, or K crops of one shape out of a few containers, in one call: entry e is a box
 * of container which[e], every entry with the same box dims, and the chunks of all entries are decoded together (one
 * chain of per-plane launches for the call, not one per box).  The containers lie anywhere in device memory -- an
 * array of pointers and lengths names them, nothing is copied together -- and only the chunks some box meets are
 * read.  A chunk that several entries meet is decoded once: such a call decodes into a staging array the library
 * keeps (sperrhip_release() frees it) and one more kernel moves every box's pieces out of it; a call whose entries
 * share no chunk writes d_dst directly.  With `level` the boxes are cut from that level of the hierarchy, origins
 * and dims in its coordinates, as sperrhip_decompress_level_dev takes them.  Box e of the result is bit for bit
 * what sperrhip_decompress_portion_dev gives for container which[e] with the same level, box and pct.
 * Both calls return -1, the second with d_dst as it was, for: nbox or ncont of 0, a NULL pointer (`which` and `level`
 * may be NULL), a `which` index >= ncont, which == NULL with nbox != ncont, a box extent of 0, a box that leaves its
 * volume or level, containers whose volume dims differ, with a level containers whose chunk dims differ or that
 * have no such level, nbox * box_dims[2] or the staging array's z extent (the sum of the z extents of the distinct
 * chunks) beyond INT32_MAX, more than 2^32 - 1 (entry, chunk) pairs, an output that is too small, or a container
 * sperrhip_decompress_dev refuses.  One container passed under two indices counts as two. */
/* host only: what a call would do.  out[5] = {slots, pairs, staged (0/1), staging values, output values}: the
 * distinct (container, chunk) pairs decoded, the (entry, chunk) pairs written, whether the call stages.
 * 0 ok, -1 for anything sperrhip_decompress_boxes_dev refuses that can be known from dims alone. */
int sperrhip_boxes_plan(size_t ncont, const size_t vol_dims[3], const size_t* chunk_dims /* 3*ncont */,
                        const uint32_t* which, const size_t* box_lo /* 3*nbox */, size_t nbox,
                        const size_t box_dims[3], const size_t* level, size_t out[5]);
/* d_srcs, src_lens: host arrays of ncont device pointers and byte lengths.
 * entry e: the box [box_lo[3e..], + box_dims) of container which[e] (NULL: container e), or of its level *level;
 * from the first pct percent of every chunk stream (0 or >= 100: all).  d_dst: nbox boxes back to back, x fastest. */
int sperrhip_decompress_boxes_dev(const void* const* d_srcs, const size_t* src_lens, size_t ncont,
                                  const uint32_t* which, const size_t* box_lo, size_t nbox,
                                  const size_t box_dims[3], const size_t* level, unsigned pct,
                                  int output_float, void* d_dst, size_t dst_cap_bytes, void* hip_stream);

/* ---- a batch of same-shape 2D slices, one stream each ------------------------------------------ */
/* N slices of the same (dimx, dimy) in one call, all of them coded side by side on the 2D coder: the
 * levels or time steps of a field, the frames of a detector, the z planes of a volume coded plane by
 * plane.  Stream s is byte for byte what sperrhip_compress_2d_dev makes of slice s alone, and slice s of
 * a batch decode is bit for bit sperrhip_decompress_2d_dev of stream s.  The slices are read as one
 * volume of dims (x, y, nslice) with 32-bit chunk origins: nslice must not exceed 2^32 - 1.  The batch
 * calls return -1 for nslice == 0, a zero dim, a NULL pointer, an output that is too small, decreasing
 * offsets, a stream sperrhip_decompress_2d_dev would refuse (shorter than 17 bytes) and, with
 * has_header, a header whose dims differ from the arguments'; a refusal found before decoding starts
 * leaves d_dst as it was, and compression never writes past dst_cap. */
/* Upper bound for sperrhip_compress_2d_batch_dev: nslice times sperrhip_max_compressed_size_2d; 0 for
 * nslice == 0 or if the product overflows size_t.  Host only. */
size_t sperrhip_max_compressed_size_2d_batch(size_t nslice, size_t dimx, size_t dimy, int mode, double quality);
/* nslice slices back to back in d_src, slice s at element s*dimx*dimy, x fastest (a contiguous (N, y, x)
 * array).  Writes nslice streams back to back into d_dst; out_inc_header != 0: each starts with its own
 * 10-byte header.  offsets (host, nslice + 1 entries) receives the byte ranges: stream s is
 * [offsets[s], offsets[s+1]).  Return codes as sperrhip_compress_2d_dev. */
int sperrhip_compress_2d_batch_dev(const void* d_src, int is_float, size_t nslice, size_t dimx, size_t dimy,
                                   int mode, double quality, int out_inc_header,
                                   void* d_dst, size_t dst_cap, size_t* offsets, void* hip_stream);
/* nslice streams in d_src, stream s at [offsets[s], offsets[s+1]) (host array), at any byte alignment.
 * has_header == 0: the streams are what sperr_decomp_2d takes; has_header != 0: each starts with the
 * 10-byte header, which is checked against dimx, dimy and skipped.  Mode, rate, truncation and the
 * precision of the coded data may differ from stream to stream.  d_dst receives nslice slices back to
 * back (float or double).  Returns 0 ok, -1 error. */
int sperrhip_decompress_2d_batch_dev(const void* d_src, const size_t* offsets, size_t nslice, int has_header,
                                     int output_float, size_t dimx, size_t dimy,
                                     void* d_dst, size_t dst_cap_bytes, void* hip_stream);

/* ---- missing values: masked volumes ------------------------------------------------------------ */
/* A volume with missing samples (NaNs, or a sentinel such as 1e20) becomes two things: an ordinary container of
 * the IN-FILLED volume -- every missing sample replaced by one finite value F -- which any SPERR reader decodes,
 * and a small MASK STREAM that says which samples were missing.  The dense calls themselves still define nothing
 * for non-finite input.
 *   missing  SPERRHIP_MISSING_NAN: x != x.  SPERRHIP_MISSING_ABS_GE: !(fabs(x) < threshold), the sample widened to
 *            double -- the sentinel, both infinities and NaN; threshold must be finite and > 0.
 *   F        lo and hi are the smallest and largest valid sample under the total order of the sign-magnitude bit
 *            patterns (-0.0 < +0.0); F = 0.5 * lo + 0.5 * hi in double, narrowed once to float for fp32 data; 0 when
 *            no sample is valid.  An infinite lo or hi (rule NAN only) fails the call with -1.
 *   stream   little-endian, sample index = linear index (x fastest), bit 1 = missing:
 *            bytes 0-3 "SPMK", 4 version (1), 5 kind, 6-7 zero, 8-15 n, 16-23 nmissing, 24-31 count, 32- payload.
 *            kind 0: nothing missing, no payload.  kind 1: `count` ascending uint32 positions p where
 *            bit(p) != bit(p - 1), bit(-1) = 0.  kind 2: count = ceil(n / 64) uint64 words, sample i is bit i % 64 of
 *            word i / 64, tail bits 0.  nmissing == 0 gives kind 0; otherwise kind 1 when n <= 2^32 and
 *            4 * toggles < 8 * ceil(n / 64); otherwise kind 2.
 * A stream's device pointer must be 8-byte aligned.  A stream that is handed in has its header checked (magic,
 * version, kind, n against the volume, count and the payload's length against mask_len); its payload is trusted: a
 * damaged one gives wrong samples, never a write outside the output.
 * Out of scope: views, batches, interleaved fields, 2D slices, levels and multires, the host calls and the farm. */
#define SPERRHIP_MISSING_NAN 1
#define SPERRHIP_MISSING_ABS_GE 2
/* 32 + 8 * ceil(n / 64): what any stream of n samples fits in.  Host only. */
size_t sperrhip_mask_max_size(size_t n);
/* The mask stream of the n samples at d_src into d_mask, and with d_filled the in-filled samples (NULL: none; it may
 * be d_src).  One host wait.  0 ok, *mask_len and *nmissing set; 1 when mask_cap is too small: nothing is written
 * and *mask_len is the size needed; -1 (nothing written) for a NULL pointer, n == 0, an unknown rule, a threshold
 * that is not finite and > 0, or an infinite lo / hi. */
int sperrhip_mask_make_dev(const void* d_src, int is_float, size_t n, int rule, double threshold,
                           void* d_filled /* NULL: none; may be d_src */, void* d_mask, size_t mask_cap,
                           size_t* mask_len, size_t* nmissing, void* hip_stream);
/* What stands at the missing samples of the in-filled volume.  The decode does not care: it overwrites them, and the
 * figures of sperrhip_quality_masked_dev skip them.  The mask stream is the same for every kind.
 *   SPERRHIP_FILL_MIDRANGE  F above, bit for bit: what the calls without a fill argument use.
 *   SPERRHIP_FILL_VALUE     fill_value, narrowed once to float for fp32 data; -1 when it is not finite, or not finite
 *                           after narrowing.  lo and hi are not looked at: an infinite valid sample fails nothing.
 *   SPERRHIP_FILL_SMOOTH    a pull-push fill, which puts no cliff at the mask's boundary and so compresses better.
 *                           Level 0 has the volume's dims, level l + 1 has ceil(d / 2) along each axis, L is the first
 *                           level of one cell; every operation is one IEEE double operation, no fma.
 *                           Pull, l = 0 .. L-1: a level-0 cell is known when its sample is valid, its value the sample
 *                           widened; cell (X, Y, Z) of level l + 1 sums its known children (2X + a, 2Y + b, 2Z + c)
 *                           inside level l from s = +0.0, through c, then b, then a, each ascending, and is known when
 *                           it has k > 0 of them, with value s / (double)k.  An unknown top cell becomes 0.0.  A sum
 *                           that is not finite fails the call with -1 (in the place of the midrange's lo / hi rule).
 *                           Push, l = L-1 .. 0: an unknown cell (x, y, z) of level l, per axis with coordinate i and
 *                           level l + 1's dim: P = i >> 1, Q = i odd ? min(P + 1, dim - 1) : (P == 0 ? 0 : P - 1);
 *                           t = 0.75 * v(Px, Y, Z) + 0.25 * v(Qx, Y, Z) for (Y, Z) in {Py, Qy} x {Pz, Qz}, then
 *                           u = 0.75 * t(Py, Z) + 0.25 * t(Qy, Z), then w = 0.75 * u(Pz) + 0.25 * u(Qz), every product
 *                           and sum rounded on its own.  A missing sample becomes w, narrowed once for fp32 data.
 *                           A volume of one sample is filled with 0.0.  Without d_filled nothing is pulled or refused. */
#define SPERRHIP_FILL_MIDRANGE 0
#define SPERRHIP_FILL_VALUE 1
#define SPERRHIP_FILL_SMOOTH 2
/* sperrhip_mask_make_dev of a volume of dimx * dimy * dimz samples (x fastest) with a fill kind: the smooth fill
 * needs the shape.  Return codes as that call; -1 also for an unknown fill kind, a fill_value that SPERRHIP_FILL_VALUE
 * refuses and a smooth fill's sum that is not finite, each before anything of the caller's is written.  One host wait. */
int sperrhip_mask_make_vol_dev(const void* d_src, int is_float, size_t dimx, size_t dimy, size_t dimz, int rule,
                               double threshold, int fill, double fill_value,
                               void* d_filled /* NULL: none; may be d_src */, void* d_mask, size_t mask_cap,
                               size_t* mask_len, size_t* nmissing, void* hip_stream);
/* the header of a stream on the device, read on the default stream (which does not wait for a non-blocking stream);
 * any of n, nmissing, kind may be NULL.  -1: the header is refused */
int sperrhip_mask_parse_dev(const void* d_mask, size_t mask_len, size_t* n, size_t* nmissing, int* kind);
/* the same on hip_stream: read behind everything enqueued there (NULL: the call above) */
int sperrhip_mask_parse_stream_dev(const void* d_mask, size_t mask_len, size_t* n, size_t* nmissing, int* kind,
                                   void* hip_stream);
/* d_vol holds the box [box_lo, box_lo + box_dims) of a volume of vol_dims densely (both NULL: the whole volume):
 * `value` -- its bits for doubles, (float)value for floats, NaN allowed -- is stored at the box's missing samples
 * and NOTHING else is written.  -1, nothing written: a refused stream, n != the volume's, a box that leaves it. */
int sperrhip_mask_apply_dev(void* d_vol, int is_float, const size_t vol_dims[3], const size_t box_lo[3],
                            const size_t box_dims[3] /* both NULL: d_vol is the whole volume */,
                            const void* d_mask, size_t mask_len, double value, void* hip_stream);
/* the mask as n bytes of 0 / 1 */
int sperrhip_mask_expand_dev(const void* d_mask, size_t mask_len, unsigned char* d_out, size_t n, void* hip_stream);
/* sperrhip_mask_make_dev into a buffer the library keeps, then sperrhip_compress_dev of the in-filled volume: the
 * container is byte for byte that call's.  With nothing missing it is the dense call's of d_src and the stream is 32
 * bytes.  Modes and return codes as sperrhip_compress_dev, and those of sperrhip_mask_make_dev for the mask. */
int sperrhip_compress_masked_dev(const void* d_src, int is_float, size_t dimx, size_t dimy, size_t dimz,
                                 size_t chunk_x, size_t chunk_y, size_t chunk_z, int mode, double quality,
                                 int rule, double threshold, void* d_dst, size_t dst_cap, size_t* dst_len,
                                 void* d_mask, size_t mask_cap, size_t* mask_len, size_t* nmissing, void* hip_stream);
/* the same with a fill kind (sperrhip_mask_make_vol_dev): the container is sperrhip_compress_dev's of that in-filled
 * volume.  fill = SPERRHIP_FILL_MIDRANGE is the call above, byte for byte. */
int sperrhip_compress_masked_fill_dev(const void* d_src, int is_float, size_t dimx, size_t dimy, size_t dimz,
                                      size_t chunk_x, size_t chunk_y, size_t chunk_z, int mode, double quality,
                                      int rule, double threshold, int fill, double fill_value, void* d_dst,
                                      size_t dst_cap, size_t* dst_len, void* d_mask, size_t mask_cap,
                                      size_t* mask_len, size_t* nmissing, void* hip_stream);
/* sperrhip_decompress_portion_dev (pct 0: everything; box_lo and box_dims both NULL: the whole volume), then
 * sperrhip_mask_apply_dev with the box: bit for bit the dense decode with `value` at the missing samples.  -1
 * before anything is written where the dense calls return it, for a refused stream, and when the stream's n is not
 * the container's volume.  There is no level form: a mask has no coarser level. */
int sperrhip_decompress_masked_dev(const void* d_src, size_t src_len, unsigned pct, int output_float,
                                   const size_t box_lo[3], const size_t box_dims[3], const void* d_mask,
                                   size_t mask_len, double value, void* d_dst, size_t dst_cap_bytes, void* hip_stream);
/* out[8] as sperrhip_quality_dev of the two arrays compacted to their valid samples in linear order, bit for bit.
 * -1 when no sample is valid. */
int sperrhip_quality_masked_dev(const void* d_orig, const void* d_recon, int is_float, size_t n,
                                const void* d_mask, size_t mask_len, double* out, void* hip_stream);

/* ---- relative error ------------------------------------------------------------------------- */

/* A point-wise RELATIVE bound, |x' - x| <= eps * |x| per sample, zeros and signs exact.  A volume x is an ordinary
 * container of a DOUBLE volume y in point-wise error mode, which any SPERR reader opens, and a side stream with the
 * samples' zero bits and sign bits.  The rule (sperr_amd/csrc/rel.h is its one statement, with the derivation):
 *   forward    d = (double)x.  Zero class: fabs(d) < 0x1p-1022 (+-0.0, double subnormals; no nonzero float).  Sign:
 *              d's sign bit.  Outside the zero class, E the biased exponent field of d and M its 52 mantissa bits,
 *              y = (double)((int)E - 1023) + (double)M * 0x1p-52; for fp32 data a y < -126 (a subnormal float, whose
 *              narrowing has an absolute grid) becomes -126 + 2 * (y + 126); in the zero class y is the NaN
 *              0x7ff8000000000000, which the encoder in-fills as a missing value (SPERRHIP_MISSING_NAN, the fill given)
 *   tolerance  t = eps / (1.0 + eps) - s in double, s = 0x1p-22 for fp32 data and 0x1p-40 for fp64 data; eps is
 *              refused unless it is finite, eps <= 0.5 and t >= s.  The container is mode 3 at quality t
 *   inverse    zero bit: a zero with its sign bit.  Otherwise, the source fp32 data and y' < -126:
 *              y' = -126 + 0.5 * (y' + 126); then y' clamped into [-1080, nextafter(1024, 0)],
 *              e = floor(y'), m = y' - e, ldexp(1.0 + m, (int)e), narrowed once for float output (FLT_MAX where that
 *              overflows), then the sign bit
 *   stream     "SPRL", little-endian, 8-byte aligned: 0-3 the magic | 4 version 1 | 5 is_float of the source | 6-7 0 |
 *              8-15 the bits of eps (+0.0 from sperrhip_rel_forward_dev, which states no bound) | 16-23 n |
 *              24-31 length of the zero stream | 32-39 length of the sign stream | 40-47 0 | the zero stream,
 *              padding to 8 bytes, the sign stream: two mask streams as above, bit 1 = zero class / negative
 * That is the map kind SPERRHIP_REL_LINEAR (0), the default and what every call without a kind means: y is the
 * piecewise linear interpolant of log2|x| between the powers of two.  SPERRHIP_REL_LOG (1) codes the true logarithm:
 * a larger tolerance and no kink at the powers of two, so a smaller container, much smaller on fields that are smooth
 * in the exponent.  Zero class, sign, the stretch of the subnormal floats, the un-stretch, the clamp, the narrowing and
 * the refusals are the same.  What differs, every operation an IEEE double operation rounded once in the order written
 * (no libm, no fused multiply-add), the constants and the derivation in rel.h:
 *   forward    m = 1.M folded into [sqrt(1/2), sqrt(2)) with its exponent e, s = (m - 1) / (m + 1), an 11-term
 *              Horner polynomial P in s * s; y = (double)e + s * P
 *   tolerance  t = y(1.0 + eps) - s with the same s; refused unless eps is finite, 0 < eps <= 0.5 and t >= s
 *   inverse    e = floor(y'), f = y' - e folded into (-1/2, 1/2], a degree-13 Horner polynomial Q in f * ln 2,
 *              ldexp(Q, (int)e); finite: DBL_MAX where the last rounding would overflow, +0.0 below 2^-1075
 *   stream     the same layout under the magic "SPLG".  A reader accepts either magic, takes the kind from it and
 *              checks eps against that kind's tolerance rule; a library from before this kind refuses "SPLG"
 * A portion decode (pct other than 0 or 100) carries no bound: finite values, zeros and
 * signs exact.  A side stream that is handed in has its three headers checked; its payload is trusted, as a mask's.
 * Return codes follow the masked calls: 0 ok; 1 side_cap too small, *side_len the size needed; -1, before anything
 * of the caller's is written: NULL pointers, n == 0, an unknown kind, a refused eps, a sample that is not finite, a refused side
 * stream, n against the container's volume, a container that is not a double one, a box that leaves the volume.
 * Out of scope, refused where it can be reached: samples that are not finite, rate and PSNR modes of y, views,
 * batches, fields, slices, levels and multires, the host calls and the farm, the command line tools. */
/* The map kinds.  A call named *_kind is the call beside it with the kind as one more argument; the call without it
 * means SPERRHIP_REL_LINEAR.  An unknown kind returns -1 before anything is written. */
#define SPERRHIP_REL_LINEAR 0
#define SPERRHIP_REL_LOG 1
/* t of eps.  Host only.  -1: eps is refused */
int sperrhip_rel_tolerance(double eps, int is_float, double* t);
int sperrhip_rel_tolerance_kind(double eps, int is_float, int kind, double* t);
/* 48 + 2 * sperrhip_mask_max_size(n).  Host only. */
size_t sperrhip_rel_max_size(size_t n);
/* y of the n samples at d_src into d_y (n doubles, no overlap with d_src) and the side stream into d_side.  One host
 * wait. */
int sperrhip_rel_forward_dev(const void* d_src, int is_float, size_t n, void* d_y, void* d_side, size_t side_cap,
                             size_t* side_len, size_t* nzero, size_t* nneg, void* hip_stream);
int sperrhip_rel_forward_kind_dev(const void* d_src, int is_float, size_t n, int kind, void* d_y, void* d_side,
                                  size_t side_cap, size_t* side_len, size_t* nzero, size_t* nneg, void* hip_stream);
/* d_y holds y' of the box [box_lo, box_lo + box_dims) of a volume of vol_dims densely (both NULL: the whole volume):
 * x' into d_dst, floats or doubles; d_dst may be d_y when doubles.  The map kind is the side stream's. */
int sperrhip_rel_inverse_dev(const void* d_y, const size_t vol_dims[3], const size_t box_lo[3],
                             const size_t box_dims[3], const void* d_side, size_t side_len, int output_float,
                             void* d_dst, void* hip_stream);
/* The forward map into a buffer the library keeps, then sperrhip_compress_masked_fill_dev of y with is_float = 0,
 * mode 3, quality t, SPERRHIP_MISSING_NAN and the fill given (fill_value in y's domain): the container and the zero
 * stream are byte for byte that call's.  Return codes as that call and as above. */
int sperrhip_compress_rel_dev(const void* d_src, int is_float, size_t dimx, size_t dimy, size_t dimz, size_t chunk_x,
                              size_t chunk_y, size_t chunk_z, double eps, int fill, double fill_value, void* d_dst,
                              size_t dst_cap, size_t* dst_len, void* d_side, size_t side_cap, size_t* side_len,
                              void* hip_stream);
int sperrhip_compress_rel_kind_dev(const void* d_src, int is_float, size_t dimx, size_t dimy, size_t dimz,
                                   size_t chunk_x, size_t chunk_y, size_t chunk_z, double eps, int kind, int fill,
                                   double fill_value, void* d_dst, size_t dst_cap, size_t* dst_len, void* d_side,
                                   size_t side_cap, size_t* side_len, void* hip_stream);
/* sperrhip_decompress_masked_dev's decode (pct, box) as doubles into a buffer the library keeps, then the inverse
 * of the side stream's map kind into d_dst.  One host wait more than that call. */
int sperrhip_decompress_rel_dev(const void* d_src, size_t src_len, unsigned pct, int output_float,
                                const size_t box_lo[3], const size_t box_dims[3], const void* d_side, size_t side_len,
                                void* d_dst, size_t dst_cap_bytes, void* hip_stream);
/* the headers of a side stream, read on hip_stream; any of the outputs may be NULL.  -1: the stream is refused */
int sperrhip_rel_parse_stream_dev(const void* d_side, size_t side_len, int* is_float, double* eps, size_t* n,
                                  size_t* nzero, size_t* nneg, void* hip_stream);
int sperrhip_rel_parse_stream_kind_dev(const void* d_side, size_t side_len, int* is_float, double* eps, size_t* n,
                                       size_t* nzero, size_t* nneg, int* kind, void* hip_stream);
/* out[4]: over the samples whose original is outside the zero class the largest |x' - x| / |x| in double and how
 * many have |x' - x| > eps * |x|; how many samples differ in zero class or in sign; the count of samples outside the
 * zero class.  One kernel, one host wait.  -1: a NULL pointer, n == 0, eps not finite or negative. */
int sperrhip_rel_check_dev(const void* d_orig, const void* d_recon, int is_float, size_t n, double eps, double* out,
                           void* hip_stream);

/* ---- time series ------------------------------------------------------------------------------ */

/* N time steps of one field, compressed together: an orthonormal Haar transform ACROSS the steps, point by point in
 * space, and every band of it an ordinary container of a double volume.  Consecutive steps are nearly equal, so the
 * detail bands are nearly zero.  A series of N steps is N containers back to back and a 64-byte info record; boxes,
 * portions, chunking and every container reader keep working on the bands, and one step of an 8-step group decodes
 * from 4 containers.  The rule (sperr_amd/csrc/series.h is its one statement, with the derivations):
 *   plan       levels L in 0 .. 4.  Steps 0 .. N-1 are cut into consecutive groups of 2^L; a remainder r < 2^L is cut by
 *              the binary digits of r, largest first (N = 11, L = 3: 8, 2, 1).  A group of 2^l steps gets l levels; a
 *              group of one is the step itself as a double.  levels = 0 is the plain batch
 *   bands      inside a group of g = 2^l: slot 0 the approximation a_l, slot 1 d_l, slots 2 .. 3 d_{l-1}, ..., slots
 *              g/2 .. g-1 d_1.  Band b of the series is group start + slot
 *   forward    fp64, no fused multiply-add, s = 0x1.6a09e667f3bcdp-1; fp32 samples are widened first:
 *              a = (e + o) * s, d = (e - o) * s, e and o the even and odd entries of the level below
 *   inverse    e = (a + d) * s, o = (a - d) * s; narrowed with one (float) for fp32 output
 *   needs      slot (level k, index j) covers the steps [j 2^k, (j+1) 2^k) of its group.  A decode of the steps
 *              [t0, t0 + nt) decodes exactly the bands whose cover meets it; no other container is read
 *   tolerance  |x' - x| <= tol at every sample of every step (double output; the narrowing of an fp32 output can add
 *              to it, as in mode 3): the bands of a group of 2^l are coded in mode 3 at tau_l = (tol - rho) / A_l,
 *              A_0 = 1, A_{l+1} = s (A_l + 1) (1.414, 1.707, 1.914, 2.061), rho = K_L 2^-53 max(M, tol) the rounding of
 *              the two butterflies, K = 0, 13, 28, 46, 67 for L = 0 .. 4, M the largest |sample| of the series.  Refused
 *              when rho >= tol / 2
 *   psnr       the transform is orthonormal, so the series' squared error is the sum of the bands': every band is
 *              coded by the rule of sperrhip_compress_psnr_dev with `range` the series' (or the caller's), hence the same
 *              target error.  As there, the target is the reference's estimate, not a guarantee
 *   info       64 bytes in HOST memory, little-endian: 0-3 "SPTS" | 4 version 1 | 5 levels | 6 is_float of the steps |
 *              7 kind | 8-11 N | 12-23 dimx, dimy, dimz (32 bits each) | 24-31 tol or psnr | 32-39 the range |
 *              40-47 M | 48-55 rho (0 in psnr mode) | 56-63 0
 * The transform pays when steps are close and costs when a step moves the field by a sample of its shortest waves
 * (README, DESIGN.md section 0l have the figures).  Every call returns -1 before anything is launched for a NULL
 * pointer, N = 0 or N > 2^32 - 1, levels > 4, a zero dimension, a range of steps outside the series, and the decode
 * for containers whose dims differ from the record's.
 * Out of scope, refused or not offered: a byte target over a series, fixed-rate mode, views, fields, masked and
 * relative volumes, 2D slices, levels of the spatial hierarchy, the host calls, the farm and the command line tools,
 * any wavelet other than Haar. */
#define SPERRHIP_SERIES_TOL 0
#define SPERRHIP_SERIES_PSNR 1
#define SPERRHIP_SERIES_INFO_BYTES 64
/* Host only.  The groups: *ngroups their count; with starts / group_levels (either may be NULL; `cap` entries each) the
 * first step and the level count of every group, 1 when cap is too small. */
int sperrhip_series_plan(size_t nsteps, unsigned levels, size_t* ngroups, size_t* starts, unsigned* group_levels,
                         size_t cap);
/* Host only.  need[b] = 1 for the bands a decode of [t0, t0 + nt) needs, 0 otherwise (nsteps entries); *count (may be
 * NULL) how many. */
int sperrhip_series_needs(size_t nsteps, unsigned levels, size_t t0, size_t nt, unsigned char* need, size_t* count);
/* Host only.  rho and tau[0 .. levels] of a tolerance and the largest |sample|; -1 where the compression refuses. */
int sperrhip_series_tolerance(double tol, double maxabs, unsigned levels, double* rho, double* tau);
/* Host only.  The fields of an info record; any output may be NULL.  -1: not a record. */
int sperrhip_series_parse(const void* info, size_t* nsteps, unsigned* levels, size_t dims[3], int* is_float, int* kind,
                          double* quality, double* range, double* maxabs, double* rho);
/* Stage access: the two kernels alone.  d_steps, d_outs: HOST arrays of device pointers, one per step (of the range);
 * every volume holds n samples and needs the alignment of its type only.  d_bands: nsteps dense volumes of n doubles,
 * band b at element b * n.  The inverse reads only the bands the range needs -- the others count as zero -- and writes
 * only the nt outputs.  No step and no output may overlap d_bands: such a call returns -1.  Both wait for the stream. */
int sperrhip_series_forward_dev(const void* const* d_steps, int is_float, size_t nsteps, unsigned levels, size_t n,
                                void* d_bands, void* hip_stream);
int sperrhip_series_inverse_dev(const void* d_bands, size_t nsteps, unsigned levels, size_t n, size_t t0, size_t nt,
                                int output_float, void* const* d_outs, void* hip_stream);
/* nsteps containers back to back in d_dst, container b -- band b -- at [offsets[b], offsets[b + 1]) (offsets: host,
 * nsteps + 1 entries), and the info record (64 bytes, host).  kind SPERRHIP_SERIES_TOL: quality is tol; container b is
 * byte for byte sperrhip_compress_dev of band b as a double volume in mode 3 at its tau.  SPERRHIP_SERIES_PSNR: quality
 * is the target in dB and range the common range (0: the series' own, max - min over all steps); container b is byte
 * for byte sperrhip_compress_psnr_dev of band b with that range.  dst_cap as sperrhip_max_compressed_size_batch(nsteps,
 * ..., 3 or 2, quality) says.  The bands are staged in a buffer the library keeps (sperrhip_release() frees it) of at
 * most SPERR_HIP_SERIES_MAX_MB MiB (default 2048): a longer series runs in windows of whole groups, a single group
 * larger than the cap is taken whole, and the containers do not depend on the cap.  -1 also for a NaN or an infinity
 * in a step, a tol that is not positive and finite or within 2 rho of zero, a psnr that is not finite, a range that
 * is negative or not finite; other return codes as sperrhip_compress_batch_dev. */
int sperrhip_compress_series_dev(const void* const* d_steps, int is_float, size_t nsteps, size_t dimx, size_t dimy,
                                 size_t dimz, size_t chunk_x, size_t chunk_y, size_t chunk_z, unsigned levels, int kind,
                                 double quality, double range, void* d_dst, size_t dst_cap, size_t* offsets, void* info,
                                 void* hip_stream);
/* The steps [t0, t0 + nt) of the series that `info` and the containers at d_src + offsets[b] describe, whole or the
 * box [box_lo, box_lo + box_dims) (both NULL: whole), from the first pct percent of every chunk stream (0 or >= 100:
 * all), as floats or doubles into the nt device pointers of d_outs (a host array), each a dense volume or box.  Only
 * the needed bands are decoded -- as doubles into the library's buffer, by the body of sperrhip_decompress_boxes_dev --,
 * then the inverse kernel runs: after any refusal or decoder error the outputs are as they were. */
int sperrhip_decompress_series_dev(const void* info, const void* d_src, const size_t* offsets, size_t t0, size_t nt,
                                   const size_t box_lo[3], const size_t box_dims[3], unsigned pct, int output_float,
                                   void* const* d_outs, void* hip_stream);

/* ---- profiling ------------------------------------------------------------------------------ */

/* When enabled, the engine brackets every pipeline stage with HIP events on the launch stream
 * and accumulates their durations. */
void sperrhip_profile_enable(int on);
/* Restrict the bracketing to one kernel (a name sperrhip_profile_get reported; NULL or "" = all):
 * two event records per launch of every kernel cost a few percent of a step. */
void sperrhip_profile_only(const char* kernel);
void sperrhip_profile_reset(void);
/* Fills up to `cap` entries; returns the number of stages. names[i] points to a static string.
 * millis: time during which the kernel was running (decoding enqueues sub-batches on several
 * streams, whose launches of one kernel overlap; for everything else this is the sum of the
 * launch durations). */
int sperrhip_profile_get(const char** names, double* millis, int* launches, int cap);
/* Same, plus the plain sum of the launch durations (sum / launches = what a kernel trace
 * reports as the average duration); sum_millis may be NULL. */
int sperrhip_profile_get2(const char** names, double* busy_millis, double* sum_millis,
                          int* launches, int cap);

/* Diagnostics of the table-driven LIS decoder: when `on`, thread 0 of every decoding workgroup
 * accumulates shader-clock ticks per phase; out64 (64 entries, may be NULL) receives the counters
 * of chunk 0 of the last decoded batch: [0..10] load, tables, hopS, P1, P2, P3, P4, expand,
 * compaction, windows, placement; [16+K] windows, [32+K] table ticks and [48+K] stream bits of
 * the list levels whose class chain has length K. */
void sperrhip_debug_lis_stamps(int on, unsigned long long* out64);

/* Diagnostics: how often this process took one of the workspace-saving paths (for the tests that
 * have to know they ran): 0 = 64-bit retries of a batch whose coder arrays lay over the chunk buffer
 * (the batch is transformed again), 1 = compression batches with the coder arrays over the chunk
 * buffer, 2 = decompression batches with a compact chunk buffer, 3 = bytes of the largest workspace
 * arena an engine of this process holds right now, 4 / 5 = bytes of pinned staging memory / of device
 * buffers the chunk farm's workers hold right now (all devices), 7 = compression batches whose 32-bit
 * pass took the fused encoder head (quantiser, leaf level of the pyramid and census in one kernel;
 * SPERR_HIP_ENC_FUSED_HEAD=0 switches it off), 8 = windows of bands the series compression calls ran (one per call
 * unless SPERR_HIP_SERIES_MAX_MB cuts it).  Other values: 0. */
unsigned long long sperrhip_debug_counter(int which);

/* Gives back what the library keeps between calls (it keeps workspaces, shape tables, pinned staging
 * buffers and device buffers so that the next call does not pay for them again): everything held by
 * engines and farm workers that are idle, and the calling thread's slice buffers.  Calls running on
 * other threads are not disturbed.  For hosts that embed the library and call it rarely (an HDF5
 * filter in a long-running service); never needed for correctness. */
void sperrhip_release(void);

/* Library/engine identification, e.g. "sperr_hip 0.1 (gfx950)". */
const char* sperrhip_version(void);

#ifdef __cplusplus
}
#endif
#endif
