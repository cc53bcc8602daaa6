// The map on the device (row o-2): a store of keyframe landmark records that outlives the window, and its export as a filtered,
// coloured point cloud.  What the reference keeps in its track and shows through its viewer and exporter:
//   PhotometricBundleAdjustment::updateFrame, the landmark rules        src/energy/problems/src/photometric_bundle_adjustment.cpp:223-263
//   ActiveTrackingLandmark::marginalize / semanticTypeId               src/track/landmarks/src/active_tracking_landmark.cpp:55-63, 71-88
//   Frame::buildPoints / validForVisualization / getColor              src/track/frames/src/frame.cpp:19-82, 190-216
//   initializeVisiblePointsStorage                                     src/output/visualizer/src/local_track.cpp:139-158
//   the exporter's loop (world transform, confident filter)            pydsopp/utils/point_cloud_exporter.py:83-107
// include/dsopp_hip.h states the rules and the arithmetic; tests/point_cloud_model.py is their NumPy statement, and the kernels are held to
// it exactly — positions bit for bit (-ffp-contract=off: every binary64 step below is a single IEEE operation).
//
// Store.  A keyframe's records live in two device arrays: 5 doubles {u, v, idepth, variance, relative_baseline} and one 8-byte word
// {flags, type, r, g, b, 0, 0, 0} per record, index = the caller's landmark index of the window.
//
// Update: ONE launch (mapUpdateKernel) over all landmarks of all window frames the map knows, a thread per landmark; the frames' pointers
// travel in the kernel's arguments.  A thread is the only writer of its record.
//
// Export: TWO launches whatever the number of keyframes, over a device table of keyframe descriptors.  The records of the exported
// keyframes are cut into chunks of 256 that never straddle two keyframes; workgroup = chunk, thread = record.
//  1 mapExportCountKernel: the predicate per record, counted by wave ballot; the chunk's count goes to memory and the workgroup draws a
//    ticket.  The workgroup that draws the last one scans the chunk counts (256 at a time, looping over more), leaves every chunk's offset
//    and writes the total and the per-keyframe counts into pinned host memory.  Integers only; no workgroup waits for another.
//  2 mapExportWriteKernel: the predicate again, the record's rank in its chunk by ballot prefix, and the outputs at chunk offset + rank
//    while that is below the capacity.  The chunk's colours are gathered in LDS and leave as aligned words (debug_views.hip's stores);
//    the few bytes in front of the first and behind the last aligned word of the chunk's range leave byte by byte.
#include "common.hpp"
#include "point_cloud.hpp"
#include "pyramid.hpp"
#include "semantic_type.hpp"

#include <cfloat>
#include <climits>
#include <cmath>
#include <map>
#include <memory>

namespace dsopp_hip {
namespace {

constexpr int kBlock = 256;              // threads of a workgroup = records of a chunk
constexpr int kWaves = kBlock / 64;
constexpr int kRecF64 = 5;               // u, v, idepth, variance, relative_baseline
constexpr uint8_t kRecMarginalized = DSOPP_HIP_MAP_FLAG_MARGINALIZED, kRecOutlier = DSOPP_HIP_MAP_FLAG_OUTLIER;
constexpr uint8_t kWinMarginalized = 1, kWinOutlier = 2;  // the window's landmark flag bits (pba_types.hpp)
constexpr double kIdepthEps = 1e-8;                       // kIdepthEps of updateFrame
constexpr double kMaxRelativeIdepthVariance = 1e-3;       // marginalize()
constexpr double kMinHomogeneous = 1e-16;                 // the exporter's skip

/** one window frame of an update */
struct MapUpdateJob {
  const double *uv, *idepth, *inv_hdd, *relative_baseline;  // the window's, the device's landmark order
  const uint8_t *flags;
  const int *to_internal;   // caller index -> device index (nullptr: identity)
  const uint8_t *hist;      // n x 256 class counters, the caller's order (nullptr: the type stays 0)
  double *rec;              // the keyframe's records
  unsigned long long *bytes;
  const uint8_t *image;     // the kept image (nullptr: none)
  int width, height, channels;
  int n, n_seen;            // the window's landmarks | the records the map held before this update
  int first_block;
};

struct MapUpdateArgs {
  MapUpdateJob job[DSOPP_HIP_MAX_FRAMES];
  int n_jobs;
  int estimate_uncertainty;
  double channels;  // C
  const unsigned long long *weights;  // 256 or nullptr
};

__global__ void __launch_bounds__(kBlock) mapUpdateKernel(MapUpdateArgs a) {
  int j = 0;
  for (int i = 1; i < a.n_jobs; ++i)
    if (a.job[i].first_block <= static_cast<int>(blockIdx.x)) j = i;
  const MapUpdateJob &job = a.job[j];
  const int c = (static_cast<int>(blockIdx.x) - job.first_block) * kBlock + static_cast<int>(threadIdx.x);
  if (c >= job.n) return;
  const int p = job.to_internal ? glb(job.to_internal)[c] : c;
  const double w_idepth = glb(job.idepth)[p];
  const unsigned w_flags = glb(job.flags)[p];
  GlobalPtr<double> rec = glb(job.rec) + static_cast<size_t>(kRecF64) * c;
  GlobalPtr<unsigned long long> word = glb(job.bytes) + c;
  double idepth, variance, baseline;
  unsigned flags, type, r, g, b;
  if (c >= job.n_seen) {  // 1 a new record
    const double u = glb(job.uv)[2 * p], v = glb(job.uv)[2 * p + 1];
    rec[0] = u;
    rec[1] = v;
    idepth = w_idepth;
    variance = DBL_MAX;
    baseline = 0.0;
    flags = 0;
    type = 0;
    r = g = b = 0;
    if (job.image && u >= 0.0 && u < static_cast<double>(job.width) && v >= 0.0 && v < static_cast<double>(job.height)) {
      const size_t px = static_cast<size_t>(static_cast<int>(v)) * job.width + static_cast<int>(u);
      GlobalPtr<const uint8_t> img = glb(job.image);
      if (job.channels == 3) {  // BGR
        b = img[3 * px], g = img[3 * px + 1], r = img[3 * px + 2];
      } else {
        r = g = b = img[px];
      }
    }
  } else {
    idepth = rec[2];
    variance = rec[3];
    baseline = rec[4];
    const unsigned long long w = *word;
    flags = w & 255u, type = (w >> 8) & 255u, r = (w >> 16) & 255u, g = (w >> 24) & 255u, b = (w >> 32) & 255u;
  }
  if (w_flags & kWinOutlier) flags |= kRecOutlier;  // 2 (:229-231)
  if (!(w_flags & kWinMarginalized)) {              // 3 (:232-260)
    if (fabs(w_idepth) < kIdepthEps)
      idepth = 0.0;
    else if (w_idepth < 0.0)
      flags |= kRecOutlier;
    else
      idepth = w_idepth;
    variance = a.estimate_uncertainty ? glb(job.inv_hdd)[p] * a.channels : 1e-5;
    const double w_baseline = glb(job.relative_baseline)[p];
    if (w_baseline > baseline) baseline = w_baseline;
  } else if (!(flags & kRecMarginalized)) {         // 4 marginalize() (active_tracking_landmark.cpp:55-63)
    if (variance / idepth > kMaxRelativeIdepthVariance || idepth < 0.0) flags |= kRecOutlier;
    flags |= kRecMarginalized;
  }
  if (job.hist) type = semanticTypeOfRow(job.hist + static_cast<size_t>(c) * kSemClasses, a.weights);  // 5
  rec[2] = idepth;
  rec[3] = variance;
  rec[4] = baseline;
  *word = static_cast<unsigned long long>(flags) | (static_cast<unsigned long long>(type) << 8) | (static_cast<unsigned long long>(r) << 16) |
          (static_cast<unsigned long long>(g) << 24) | (static_cast<unsigned long long>(b) << 32);
}

/** one keyframe of an export */
struct MapKeyframeDev {
  const double *rec;
  const unsigned long long *bytes;
  int n, first_chunk;
  double ifx, ify, cx, cy;  // 1 / fx, 1 / fy
  double R[9], t[3];        // T_world_agent
};

struct MapExportArgs {
  const MapKeyframeDev *kf;
  int n_kf, n_chunks;
  int classes, apply_filters, frame, colours;
  double min_relative_baseline, max_idepth_variance, min_relative_baseline_filter;
  long long capacity;
  unsigned *chunk_count, *chunk_offset, *ticket;
  long long *count_out;  // pinned
  int *per_kf_out;       // pinned
  double *xyz, *relative_baseline, *idepth_variance;
  uint8_t *rgb, *type;
  int *keyframe_index, *record_index;
};

/** the keyframe of a chunk: the last one whose first chunk is not behind it (keyframes without records share their successor's) */
__device__ __forceinline__ int keyframeOfChunk(const MapKeyframeDev *kf, int n_kf, int chunk) {
  int lo = 0, hi = n_kf - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (kf[mid].first_chunk <= chunk)
      lo = mid;
    else
      hi = mid - 1;
  }
  return lo;
}

/** validForVisualization by class mask, then the two strict filters, then the exporter's skip */
__device__ __forceinline__ bool exported(const MapExportArgs &a, double idepth, double variance, double baseline, unsigned flags) {
  const bool required = idepth != 0.0 && baseline > a.min_relative_baseline;
  const int cls = (flags & kRecOutlier) ? DSOPP_HIP_MAP_CLASS_OUTLIER
                                        : (flags & kRecMarginalized) ? DSOPP_HIP_MAP_CLASS_MARGINALIZED : DSOPP_HIP_MAP_CLASS_ACTIVE;
  bool pass = required && (a.classes & cls) != 0;
  if (a.apply_filters) pass = pass && variance < a.max_idepth_variance && baseline > a.min_relative_baseline_filter;
  if (a.frame == DSOPP_HIP_MAP_FRAME_WORLD) pass = pass && !(fabs(idepth) < kMinHomogeneous);
  return pass;
}

struct ChunkRecord {
  bool pass;
  int k, i;  // keyframe of the export, record of the keyframe
  double u, v, idepth, variance, baseline;
  unsigned long long word;
};

__device__ __forceinline__ ChunkRecord loadChunkRecord(const MapExportArgs &a, const MapKeyframeDev &kf, int k) {
  ChunkRecord rc;
  rc.k = k;
  rc.i = (static_cast<int>(blockIdx.x) - kf.first_chunk) * kBlock + static_cast<int>(threadIdx.x);
  rc.pass = false;
  if (rc.i < kf.n) {
    GlobalPtr<const double> rec = glb(kf.rec) + static_cast<size_t>(kRecF64) * rc.i;
    rc.u = rec[0], rc.v = rec[1], rc.idepth = rec[2], rc.variance = rec[3], rc.baseline = rec[4];
    rc.word = glb(kf.bytes)[rc.i];
    rc.pass = exported(a, rc.idepth, rc.variance, rc.baseline, static_cast<unsigned>(rc.word & 255u));
  }
  return rc;
}

/** inclusive sum over the wave's lanes */
__device__ __forceinline__ unsigned waveInclusive(unsigned v, unsigned lane) {
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned o = __shfl_up(v, off);
    if (lane >= static_cast<unsigned>(off)) v += o;
  }
  return v;
}

__global__ void __launch_bounds__(kBlock) mapExportCountKernel(MapExportArgs a) {
  __shared__ unsigned lds_wave[kWaves];
  __shared__ unsigned s_last;
  const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = keyframeOfChunk(a.kf, a.n_kf, static_cast<int>(blockIdx.x));
  const ChunkRecord rc = loadChunkRecord(a, a.kf[k], k);
  const unsigned long long ballot = __ballot(rc.pass);
  if (lane == 0) lds_wave[wave] = static_cast<unsigned>(__popcll(ballot));
  __syncthreads();
  if (tid == 0) {
    unsigned total = 0;
    for (int w = 0; w < kWaves; ++w) total += lds_wave[w];
    __hip_atomic_store(&a.chunk_count[blockIdx.x], total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __atomic_thread_fence(__ATOMIC_RELEASE);  // (device scope: the count above is visible before the ticket)
    s_last = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1u : 0u;
  }
  __syncthreads();
  if (!s_last) return;
  // the last workgroup: every chunk's count is in memory; an exclusive scan, 256 chunks at a time
  unsigned base = 0;
  const unsigned n_chunks = static_cast<unsigned>(a.n_chunks);
  for (unsigned first = 0; first < n_chunks; first += kBlock) {
    const unsigned chunk = first + tid;
    const unsigned count = chunk < n_chunks ? __hip_atomic_load(&a.chunk_count[chunk], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
    const unsigned incl = waveInclusive(count, lane);
    __syncthreads();  // (the previous round's wave sums were read)
    if (lane == 63) lds_wave[wave] = incl;
    __syncthreads();
    unsigned before = 0, round = 0;
    for (unsigned w = 0; w < kWaves; ++w) {
      if (w < wave) before += lds_wave[w];
      round += lds_wave[w];
    }
    if (chunk < n_chunks) __hip_atomic_store(&a.chunk_offset[chunk], base + before + incl - count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    base += round;
  }
  __threadfence();
  __syncthreads();  // the offsets are in memory: a keyframe's count is the distance between its first chunk's offset and its successor's
  for (int q = static_cast<int>(tid); q < a.n_kf; q += kBlock) {
    const int c0 = a.kf[q].first_chunk, c1 = q + 1 < a.n_kf ? a.kf[q + 1].first_chunk : a.n_chunks;
    const unsigned o0 = c0 < a.n_chunks ? __hip_atomic_load(&a.chunk_offset[c0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : base;
    const unsigned o1 = c1 < a.n_chunks ? __hip_atomic_load(&a.chunk_offset[c1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : base;
    a.per_kf_out[q] = static_cast<int>(o1 - o0);
  }
  if (tid == 0) {
    *a.count_out = static_cast<long long>(base);
    __hip_atomic_store(a.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // armed for the next launch
  }
}

// kSemanticColors (frame.cpp:19-26) as r | g << 8 | b << 16
__device__ const unsigned kSemanticRgb[14] = {
    200u | 200u << 8 | 200u << 16, 71u | 71u << 8 | 107u << 16,   255u | 77u << 8 | 210u << 16,  255u | 255u << 8 | 153u << 16,
    255u | 0u << 8 | 0u << 16,     51u | 51u << 8 | 153u << 16,   224u | 224u << 8 | 235u << 16, 255u | 255u << 8 | 0u << 16,
    127u | 127u << 8 | 127u << 16, 0u | 255u << 8 | 0u << 16,     0u | 0u << 8 | 255u << 16,     102u | 51u << 8 | 0u << 16,
    51u | 102u << 8 | 153u << 16,  139u | 0u << 8 | 255u << 16};

/** r | g << 8 | b << 16 of a record under the export's colour scheme (getColor, frame.cpp:53-82; the exporter's image colours) */
__device__ __forceinline__ unsigned colourOf(int scheme, unsigned long long word) {
  const unsigned flags = word & 255u, type = (word >> 8) & 255u;
  if (scheme == DSOPP_HIP_MAP_COLOURS_LANDMARK_TYPE) {
    if (flags & kRecOutlier) return 255u;
    if (flags & kRecMarginalized) return 255u | 100u << 8 | 100u << 16;
    return 100u | 255u << 8 | 100u << 16;
  }
  if (scheme == DSOPP_HIP_MAP_COLOURS_SEMANTIC) return kSemanticRgb[type % 14u];
  if (scheme == DSOPP_HIP_MAP_COLOURS_IMAGE) return static_cast<unsigned>((word >> 16) & 0xffffffu);
  return 200u | 200u << 8 | 200u << 16;
}

__global__ void __launch_bounds__(kBlock) mapExportWriteKernel(MapExportArgs a) {
  __shared__ unsigned lds_wave[kWaves];
  __shared__ __attribute__((aligned(4))) uint8_t lds_rgb[3 * kBlock + 4];
  const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int k = keyframeOfChunk(a.kf, a.n_kf, static_cast<int>(blockIdx.x));
  const MapKeyframeDev &kf = a.kf[k];
  const ChunkRecord rc = loadChunkRecord(a, kf, k);
  const unsigned long long ballot = __ballot(rc.pass);
  if (lane == 0) lds_wave[wave] = static_cast<unsigned>(__popcll(ballot));
  __syncthreads();
  unsigned local = static_cast<unsigned>(__popcll(ballot & ((1ull << lane) - 1ull))), chunk_total = 0;
  for (unsigned w = 0; w < kWaves; ++w) {
    if (w < wave) local += lds_wave[w];
    chunk_total += lds_wave[w];
  }
  const long long offset = static_cast<long long>(a.chunk_offset[blockIdx.x]);
  if (offset >= a.capacity) return;  // (uniform)
  const unsigned kept = a.capacity - offset < static_cast<long long>(chunk_total) ? static_cast<unsigned>(a.capacity - offset) : chunk_total;
  const bool writes = rc.pass && local < kept;
  if (writes) {
    const size_t dest = static_cast<size_t>(offset) + local;
    if (a.xyz) {
      // d = ((u - cx) (1 / fx), (v - cy) (1 / fy), 1)  (frame.cpp:152, pinhole_camera.hpp:137-139)
      const double dx = (rc.u - kf.cx) * kf.ifx, dy = (rc.v - kf.cy) * kf.ify;
      double x, y, z;
      if (a.frame == DSOPP_HIP_MAP_FRAME_WORLD) {  // (R d + t idepth) / idepth  (point_cloud_exporter.py:96-101)
        const double px = ((kf.R[0] * dx + kf.R[1] * dy) + kf.R[2]) + kf.t[0] * rc.idepth;
        const double py = ((kf.R[3] * dx + kf.R[4] * dy) + kf.R[5]) + kf.t[1] * rc.idepth;
        const double pz = ((kf.R[6] * dx + kf.R[7] * dy) + kf.R[8]) + kf.t[2] * rc.idepth;
        x = px / rc.idepth, y = py / rc.idepth, z = pz / rc.idepth;
      } else {
        x = dx / rc.idepth, y = dy / rc.idepth, z = 1.0 / rc.idepth;
      }
      GlobalPtr<double> o = glb(a.xyz) + 3 * dest;
      o[0] = x, o[1] = y, o[2] = z;
    }
    if (a.type) glb(a.type)[dest] = static_cast<uint8_t>((rc.word >> 8) & 255u);
    if (a.relative_baseline) glb(a.relative_baseline)[dest] = rc.baseline;
    if (a.idepth_variance) glb(a.idepth_variance)[dest] = rc.variance;
    if (a.keyframe_index) glb(a.keyframe_index)[dest] = rc.k;
    if (a.record_index) glb(a.record_index)[dest] = rc.i;
  }
  if (!a.rgb) return;  // (uniform)
  if (writes) {
    const unsigned c = colourOf(a.colours, rc.word);
    lds_rgb[3 * local] = static_cast<uint8_t>(c), lds_rgb[3 * local + 1] = static_cast<uint8_t>(c >> 8), lds_rgb[3 * local + 2] = static_cast<uint8_t>(c >> 16);
  }
  __syncthreads();
  // the chunk's bytes [g0, g1) of the output: aligned words in [a0, a1), single bytes in front and behind (their words' other bytes belong
  // to the neighbouring chunks)
  const size_t g0 = 3 * static_cast<size_t>(offset), g1 = g0 + 3 * static_cast<size_t>(kept);
  size_t a0 = (g0 + 3) & ~static_cast<size_t>(3), a1 = g1 & ~static_cast<size_t>(3);
  if (a0 > a1) a0 = a1 = g1;  // (no aligned word inside: all bytes singly)
  const size_t head = (a0 < g1 ? a0 : g1) - g0;  // 0 .. 3 bytes, or all of them
  const unsigned words = static_cast<unsigned>((a1 - a0) / 4);
  if (tid < words) {
    const unsigned l = static_cast<unsigned>(head) + 4 * tid;
    const unsigned w = lds_rgb[l] | (static_cast<unsigned>(lds_rgb[l + 1]) << 8) | (static_cast<unsigned>(lds_rgb[l + 2]) << 16) |
                       (static_cast<unsigned>(lds_rgb[l + 3]) << 24);
    *reinterpret_cast<GlobalPtr<unsigned>>(glb(a.rgb) + a0 + 4 * static_cast<size_t>(tid)) = w;
  }
  const unsigned tail_first = static_cast<unsigned>(head) + 4 * words, n_bytes = 3 * kept;
  const unsigned singles = static_cast<unsigned>(head) + (n_bytes - tail_first);  // at most 3 + 3 (or all bytes of a tiny range)
  const unsigned s = tid - words;  // threads behind the word writers
  if (tid >= words && s < singles) {
    const unsigned l = s < head ? s : tail_first + (s - static_cast<unsigned>(head));
    reinterpret_cast<GlobalPtr<volatile uint8_t>>(glb(a.rgb))[g0 + l] = lds_rgb[l];
  }
}

/** (qx, qy, qz, qw) -> R, row-major, by the formula of synthetic.params_to_mat, single binary64 steps in its order */
void rotationOf(const double *q, double *R) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  R[0] = 1.0 - 2.0 * (y * y + z * z), R[1] = 2.0 * (x * y - z * w), R[2] = 2.0 * (x * z + y * w);
  R[3] = 2.0 * (x * y + z * w), R[4] = 1.0 - 2.0 * (x * x + z * z), R[5] = 2.0 * (y * z - x * w);
  R[6] = 2.0 * (x * z - y * w), R[7] = 2.0 * (y * z + x * w), R[8] = 1.0 - 2.0 * (x * x + y * y);
}

struct Keyframe {
  int id = 0;
  bool live = false;       // still fed by a window (add_keyframe); false: finalised, or loaded by set_records
  bool has_image = false;  // its colours were sampled from an image (or given)
  int n = 0;
  double intr[4] = {1, 1, 0, 0};
  double T[7] = {0, 0, 0, 1, 0, 0, 0};
  DeviceBuffer<double> rec;
  DeviceBuffer<unsigned long long> bytes;
  DeviceMem<uint8_t> image;  // the kept 8-bit image while live
  int width = 0, height = 0, channels = 0;
};

/** everything enqueued on `consumer` after this call runs behind what `producer` holds now */
void orderBehind(Event &e, hipStream_t producer, hipStream_t consumer) {
  if (producer == consumer) return;
  HIP_CHECK(hipEventRecord(e.get(hipEventDisableTiming), producer));
  HIP_CHECK(hipStreamWaitEvent(consumer, e.h, 0));
}

}  // namespace
}  // namespace dsopp_hip

using namespace dsopp_hip;

struct dsopp_hip_map {
  StreamRef sr;
  dsopp_hip_map_options opt;
  std::vector<std::unique_ptr<Keyframe>> keyframes;  // insertion order
  std::map<int, size_t> index;                       // id -> position
  DeviceMem<unsigned long long> weights;             // 256 words, allocated by the first update that gives weights
  Event window_done, update_done, pyramid_done;
  // export
  PinnedMem<char> h_table;         // the keyframe descriptors as uploaded
  PinnedMem<char> h_result;        // [count | per-keyframe counts]
  DeviceBuffer<MapKeyframeDev> d_table;
  DeviceBuffer<unsigned> d_chunks;  // [ticket, pad 3 | counts | offsets]
  DeviceBuffer<uint8_t> d_out;      // the host form's outputs
  bool in_flight = false;           // an export of the device form may still read h_table / write h_result

  Keyframe *find(int id) {
    const auto it = index.find(id);
    return it == index.end() ? nullptr : keyframes[it->second].get();
  }
  Keyframe &byId(int id) {
    Keyframe *k = find(id);
    if (!k) fail(DSOPP_HIP_ERR_NOT_FOUND, "keyframe %d is not in the map", id);
    return *k;
  }
  Keyframe &append(int id) {
    keyframes.push_back(std::make_unique<Keyframe>());
    index[id] = keyframes.size() - 1;
    keyframes.back()->id = id;
    return *keyframes.back();
  }
  void settle() {
    if (in_flight) sr.sync();
    in_flight = false;
  }
  void finalise(Keyframe &k) {
    if (k.image) {
      sr.sync();  // (an update that samples the image may be in flight)
      k.image.reset();
    }
    k.live = false;
  }

  struct ExportOutputs {
    double *xyz = nullptr, *relative_baseline = nullptr, *idepth_variance = nullptr;
    uint8_t *rgb = nullptr, *type = nullptr;
    int *keyframe_index = nullptr, *record_index = nullptr;
  };
  struct ExportPlan {
    int n_kf = 0, n_chunks = 0;
    long long total = 0;  // records of the exported keyframes
  };

  static void checkExportOptions(const dsopp_hip_map_export_options *o, int32_t n_ids, const int32_t *ids, int64_t capacity) {
    if (!o) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null export options");
    if (o->classes < 0 || o->classes > (DSOPP_HIP_MAP_CLASS_ACTIVE | DSOPP_HIP_MAP_CLASS_MARGINALIZED | DSOPP_HIP_MAP_CLASS_OUTLIER))
      fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "class mask %d", o->classes);
    if (o->frame != DSOPP_HIP_MAP_FRAME_KEYFRAME && o->frame != DSOPP_HIP_MAP_FRAME_WORLD) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "frame %d", o->frame);
    if (o->colours < DSOPP_HIP_MAP_COLOURS_LANDMARK_TYPE || o->colours > DSOPP_HIP_MAP_COLOURS_IMAGE)
      fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "colour scheme %d", o->colours);
    if (n_ids < 0 || capacity < 0) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "%d ids, capacity %lld", n_ids, static_cast<long long>(capacity));
    if (n_ids > 0 && !ids) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null id list");
  }

  /** the descriptor table of the exported keyframes, uploaded; the chunk arrays sized */
  ExportPlan plan(const dsopp_hip_map_export_options &o, int32_t n_ids, const int32_t *ids) {
    std::vector<Keyframe *> list;
    if (ids) {
      for (int i = 0; i < n_ids; ++i) list.push_back(&byId(ids[i]));
    } else {
      for (auto &k : keyframes) list.push_back(k.get());
    }
    ExportPlan p;
    p.n_kf = static_cast<int>(list.size());
    if (o.colours == DSOPP_HIP_MAP_COLOURS_IMAGE)
      for (const Keyframe *k : list)
        if (!k->has_image) fail(DSOPP_HIP_ERR_STATE, "keyframe %d has no image colours", k->id);
    for (const Keyframe *k : list) p.total += k->n;
    if (p.total > INT_MAX) fail(DSOPP_HIP_ERR_CAPACITY, "%lld records in one export", p.total);
    settle();
    h_table.reserve(sizeof(MapKeyframeDev) * static_cast<size_t>(p.n_kf > 0 ? p.n_kf : 1));
    h_result.reserve(sizeof(long long) + sizeof(int) * static_cast<size_t>(p.n_kf > 0 ? p.n_kf : 1));
    MapKeyframeDev *t = reinterpret_cast<MapKeyframeDev *>(h_table.get());
    for (int q = 0; q < p.n_kf; ++q) {
      const Keyframe &k = *list[static_cast<size_t>(q)];
      MapKeyframeDev &d = t[q];
      d.rec = k.rec.ptr;
      d.bytes = k.bytes.ptr;
      d.n = k.n;
      d.first_chunk = p.n_chunks;
      p.n_chunks += (k.n + kBlock - 1) / kBlock;
      d.ifx = 1.0 / k.intr[0];
      d.ify = 1.0 / k.intr[1];
      d.cx = k.intr[2];
      d.cy = k.intr[3];
      rotationOf(k.T, d.R);
      for (int i = 0; i < 3; ++i) d.t[i] = k.T[4 + i];
    }
    *reinterpret_cast<long long *>(h_result.get()) = 0;
    std::memset(h_result.get() + sizeof(long long), 0, sizeof(int) * static_cast<size_t>(p.n_kf));
    if (p.n_chunks > 0) {
      hipStream_t st = sr.stream;
      d_table.reserve(static_cast<size_t>(p.n_kf), 0, st);
      d_chunks.reserve(4 + 2 * static_cast<size_t>(p.n_chunks), 0, st);  // (zero-filled when it grows: the ticket; the kernel re-arms it)
      HIP_CHECK(hipMemcpyAsync(d_table.ptr, t, sizeof(MapKeyframeDev) * static_cast<size_t>(p.n_kf), hipMemcpyHostToDevice, st));
    }
    return p;
  }

  void enqueue(const dsopp_hip_map_export_options &o, const ExportPlan &p, int64_t capacity, const ExportOutputs &out, hipStream_t st) {
    if (p.n_chunks <= 0) return;
    MapExportArgs a{};
    a.kf = d_table.ptr;
    a.n_kf = p.n_kf;
    a.n_chunks = p.n_chunks;
    a.classes = o.classes;
    a.apply_filters = o.apply_filters;
    a.frame = o.frame;
    a.colours = o.colours;
    a.min_relative_baseline = opt.min_relative_baseline;
    a.max_idepth_variance = o.max_idepth_variance;
    a.min_relative_baseline_filter = o.min_relative_baseline_filter;
    a.capacity = capacity;
    a.ticket = d_chunks.ptr;
    a.chunk_count = d_chunks.ptr + 4;
    a.chunk_offset = a.chunk_count + p.n_chunks;
    a.count_out = reinterpret_cast<long long *>(h_result.get());
    a.per_kf_out = reinterpret_cast<int *>(h_result.get() + sizeof(long long));
    a.xyz = out.xyz, a.relative_baseline = out.relative_baseline, a.idepth_variance = out.idepth_variance;
    a.rgb = out.rgb, a.type = out.type;
    a.keyframe_index = out.keyframe_index, a.record_index = out.record_index;
    mapExportCountKernel<<<static_cast<unsigned>(p.n_chunks), kBlock, 0, st>>>(a);
    HIP_CHECK(hipGetLastError());
    const bool any = out.xyz || out.rgb || out.type || out.relative_baseline || out.idepth_variance || out.keyframe_index || out.record_index;
    if (any && capacity > 0) {
      mapExportWriteKernel<<<static_cast<unsigned>(p.n_chunks), kBlock, 0, st>>>(a);
      HIP_CHECK(hipGetLastError());
    }
  }

  long long countResult(int n_kf, int32_t *per_keyframe_counts) const {
    if (per_keyframe_counts && n_kf > 0) std::memcpy(per_keyframe_counts, h_result.get() + sizeof(long long), sizeof(int) * static_cast<size_t>(n_kf));
    return *reinterpret_cast<const long long *>(h_result.get());
  }
};

extern "C" {

void dsopp_hip_map_default_options(dsopp_hip_map_options *o) {
  if (!o) return;
  o->estimate_uncertainty = 1;
  o->channels = 1;
  o->min_relative_baseline = 0.1;
}

void dsopp_hip_map_default_export_options(dsopp_hip_map_export_options *o) {
  if (!o) return;
  o->classes = DSOPP_HIP_MAP_CLASS_ACTIVE | DSOPP_HIP_MAP_CLASS_MARGINALIZED;
  o->apply_filters = 0;
  o->max_idepth_variance = 5e-8;          // the exporter's (point_cloud_exporter.py)
  o->min_relative_baseline_filter = 0.15;
  o->frame = DSOPP_HIP_MAP_FRAME_WORLD;
  o->colours = DSOPP_HIP_MAP_COLOURS_LANDMARK_TYPE;
}

int dsopp_hip_map_create(int device, void *stream, const dsopp_hip_map_options *options, dsopp_hip_map **out) {
  return guarded([&] {
    if (!out) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null output");
    dsopp_hip_map_options o;
    dsopp_hip_map_default_options(&o);
    if (options) o = *options;
    if (o.channels < 1 || !(o.min_relative_baseline == o.min_relative_baseline))
      fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "%d channels, minimal relative baseline %g", o.channels, o.min_relative_baseline);
    auto m = std::make_unique<dsopp_hip_map>();
    m->sr.init(device, stream);
    m->opt = o;
    *out = m.release();
  });
}

void dsopp_hip_map_destroy(dsopp_hip_map *m) {
  if (!m) return;
  (void)hipSetDevice(m->sr.device);
  (void)hipStreamSynchronize(m->sr.stream);
  delete m;
}

int dsopp_hip_map_add_keyframe(dsopp_hip_map *m, dsopp_hip_window *window, int32_t frame_id, const dsopp_hip_pyramid *pyramid) {
  return guarded([&] {
    if (!m) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null map");
    MapWindowView view;
    mapWindowView(window, view);
    if (view.device != m->sr.device) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the window lives on device %d, the map on %d", view.device, m->sr.device);
    if (pyramid && pyramid->sr.device != m->sr.device)
      fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the pyramid lives on device %d, the map on %d", pyramid->sr.device, m->sr.device);
    const MapWindowFrame *f = nullptr;
    for (int s = 0; s < view.n_frames; ++s)
      if (view.frame[s].id == frame_id) f = &view.frame[s];
    if (!f) fail(DSOPP_HIP_ERR_NOT_FOUND, "frame %d is not in the window", frame_id);
    if (m->find(frame_id)) fail(DSOPP_HIP_ERR_STATE, "keyframe %d is in the map already", frame_id);
    m->sr.use();
    // (the image first: a failed allocation leaves the map as it was)
    DeviceMem<uint8_t> image;
    int channels = 0;
    if (pyramid && (pyramid->has_colour || pyramid->has_undistorted)) {
      channels = pyramid->has_colour ? 3 : 1;
      const size_t bytes = static_cast<size_t>(channels) * pyramid->width * pyramid->height;
      image.alloc(bytes);
      orderBehind(m->pyramid_done, pyramid->sr.stream, m->sr.stream);
      HIP_CHECK(hipMemcpyAsync(image.get(), channels == 3 ? pyramid->colour_u8.get() : pyramid->undistorted_u8.get(), bytes, hipMemcpyDeviceToDevice,
                               m->sr.stream));
      m->sr.sync();  // (the pyramid is not borrowed: it may be rebuilt as soon as this call returns)
    }
    Keyframe &k = m->append(frame_id);
    k.live = true;
    k.has_image = channels != 0;
    k.channels = channels;
    if (channels) k.width = pyramid->width, k.height = pyramid->height;
    k.image = std::move(image);
    std::memcpy(k.intr, f->intr, sizeof(k.intr));
    std::memcpy(k.T, f->T_world_agent, sizeof(k.T));
  });
}

int dsopp_hip_map_update(dsopp_hip_map *m, dsopp_hip_window *window, const uint64_t *weights256) {
  return guarded([&] {
    if (!m) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null map");
    MapWindowView view;
    mapWindowView(window, view);
    if (view.device != m->sr.device) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the window lives on device %d, the map on %d", view.device, m->sr.device);
    m->sr.use();
    hipStream_t st = m->sr.stream;
    // a keyframe the window no longer holds is finalised
    for (auto &k : m->keyframes) {
      if (!k->live) continue;
      bool held = false;
      for (int s = 0; s < view.n_frames; ++s) held = held || view.frame[s].id == k->id;
      if (!held) m->finalise(*k);
    }
    for (int s = 0; s < view.n_frames; ++s) {
      const Keyframe *k = m->find(view.frame[s].id);
      if (k && k->live && view.frame[s].n < k->n)
        fail(DSOPP_HIP_ERR_STATE, "frame %d holds %d landmarks, the map has seen %d", k->id, view.frame[s].n, k->n);
    }
    MapUpdateArgs a{};
    int blocks = 0;
    for (int s = 0; s < view.n_frames; ++s) {
      const MapWindowFrame &f = view.frame[s];
      Keyframe *k = m->find(f.id);
      if (!k || !k->live) continue;
      std::memcpy(k->intr, f.intr, sizeof(k->intr));
      std::memcpy(k->T, f.T_world_agent, sizeof(k->T));
      if (f.n <= 0) continue;
      k->rec.reserve(static_cast<size_t>(kRecF64) * f.n, static_cast<size_t>(kRecF64) * k->n, st);
      k->bytes.reserve(static_cast<size_t>(f.n), static_cast<size_t>(k->n), st);
      MapUpdateJob &j = a.job[a.n_jobs++];
      j.uv = f.uv, j.idepth = f.idepth, j.inv_hdd = f.inv_hdd, j.relative_baseline = f.relative_baseline;
      j.flags = f.flags;
      j.to_internal = f.to_internal;
      j.hist = f.sem_hist;
      j.rec = k->rec.ptr;
      j.bytes = k->bytes.ptr;
      j.image = k->image.get();
      j.width = k->width, j.height = k->height, j.channels = k->channels;
      j.n = f.n;
      j.n_seen = k->n;
      j.first_block = blocks;
      blocks += (f.n + kBlock - 1) / kBlock;
      k->n = f.n;
    }
    if (!a.n_jobs) return;
    a.estimate_uncertainty = m->opt.estimate_uncertainty;
    a.channels = static_cast<double>(m->opt.channels);
    if (weights256) {
      if (!m->weights) m->weights.alloc(kSemClasses * sizeof(unsigned long long));
      HIP_CHECK(hipMemcpyAsync(m->weights.get(), weights256, kSemClasses * sizeof(unsigned long long), hipMemcpyHostToDevice, st));
      a.weights = m->weights.get();
    }
    orderBehind(m->window_done, view.stream, st);
    mapUpdateKernel<<<static_cast<unsigned>(blocks), kBlock, 0, st>>>(a);
    HIP_CHECK(hipGetLastError());
    orderBehind(m->update_done, st, view.stream);  // (the window's next writes run behind these reads)
  });
}

int dsopp_hip_map_set_records(dsopp_hip_map *m, int32_t frame_id, const double intrinsics[4], const double T_world_agent[7], int32_t n, const double *uv,
                              const double *idepth, const double *variance, const double *relative_baseline, const uint8_t *flags, const uint8_t *type,
                              const uint8_t *rgb) {
  return guarded([&] {
    if (!m || !intrinsics || !T_world_agent) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (n < 0) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "%d records", n);
    if (n > 0 && (!uv || !idepth || !variance || !relative_baseline || !flags)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null record array");
    for (int i = 0; i < n; ++i)
      if (flags[i] & ~(kRecMarginalized | kRecOutlier)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "record %d: flags %d", i, flags[i]);
    Keyframe *k = m->find(frame_id);
    if (k && k->live) fail(DSOPP_HIP_ERR_STATE, "keyframe %d is still fed by a window", frame_id);
    m->sr.use();
    m->settle();
    hipStream_t st = m->sr.stream;
    std::vector<double> rec(static_cast<size_t>(kRecF64) * n);
    std::vector<unsigned long long> bytes(static_cast<size_t>(n));
    for (size_t i = 0; i < static_cast<size_t>(n); ++i) {
      rec[kRecF64 * i] = uv[2 * i], rec[kRecF64 * i + 1] = uv[2 * i + 1];
      rec[kRecF64 * i + 2] = idepth[i], rec[kRecF64 * i + 3] = variance[i], rec[kRecF64 * i + 4] = relative_baseline[i];
      unsigned long long w = flags[i];
      if (type) w |= static_cast<unsigned long long>(type[i]) << 8;
      if (rgb)
        w |= (static_cast<unsigned long long>(rgb[3 * i]) << 16) | (static_cast<unsigned long long>(rgb[3 * i + 1]) << 24) |
             (static_cast<unsigned long long>(rgb[3 * i + 2]) << 32);
      bytes[i] = w;
    }
    if (!k) k = &m->append(frame_id);
    k->live = false;
    k->has_image = rgb != nullptr;
    std::memcpy(k->intr, intrinsics, sizeof(k->intr));
    std::memcpy(k->T, T_world_agent, sizeof(k->T));
    k->n = 0;
    if (n > 0) {
      k->rec.reserve(rec.size(), 0, st);
      k->bytes.reserve(bytes.size(), 0, st);
      k->rec.upload(rec.data(), rec.size(), 0, st);
      k->bytes.upload(bytes.data(), bytes.size(), 0, st);
      m->sr.sync();  // (the staging vectors leave scope)
      k->n = n;
    }
  });
}

int dsopp_hip_map_set_pose(dsopp_hip_map *m, int32_t frame_id, const double T_world_agent[7]) {
  return guarded([&] {
    if (!m || !T_world_agent) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    std::memcpy(m->byId(frame_id).T, T_world_agent, sizeof(double) * 7);
  });
}

int dsopp_hip_map_num_keyframes(dsopp_hip_map *m, int32_t *n) {
  return guarded([&] {
    if (!m || !n) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    *n = static_cast<int32_t>(m->keyframes.size());
  });
}

int dsopp_hip_map_keyframe_ids(dsopp_hip_map *m, int32_t capacity, int32_t *ids, int32_t *n) {
  return guarded([&] {
    if (!m || !n || capacity < 0 || (capacity && !ids)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "bad argument");
    *n = static_cast<int32_t>(m->keyframes.size());
    for (int i = 0; i < capacity && i < *n; ++i) ids[i] = m->keyframes[static_cast<size_t>(i)]->id;
  });
}

int dsopp_hip_map_num_records(dsopp_hip_map *m, int32_t frame_id, int32_t *n) {
  return guarded([&] {
    if (!m || !n) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    *n = m->byId(frame_id).n;
  });
}

int dsopp_hip_map_get_records(dsopp_hip_map *m, int32_t frame_id, double *uv, double *idepth, double *variance, double *relative_baseline, uint8_t *flags,
                              uint8_t *type, uint8_t *rgb, double intrinsics[4], double T_world_agent[7], int32_t state[2]) {
  return guarded([&] {
    if (!m) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null map");
    Keyframe &k = m->byId(frame_id);
    if (intrinsics) std::memcpy(intrinsics, k.intr, sizeof(k.intr));
    if (T_world_agent) std::memcpy(T_world_agent, k.T, sizeof(k.T));
    if (state) state[0] = k.has_image ? 1 : 0, state[1] = k.live ? 0 : 1;
    const size_t n = static_cast<size_t>(k.n);
    if (!n || !(uv || idepth || variance || relative_baseline || flags || type || rgb)) return;
    m->sr.use();
    std::vector<double> rec(kRecF64 * n);
    std::vector<unsigned long long> bytes(n);
    k.rec.download(rec.data(), rec.size(), 0, m->sr.stream);
    k.bytes.download(bytes.data(), n, 0, m->sr.stream);
    m->sr.sync();
    for (size_t i = 0; i < n; ++i) {
      if (uv) uv[2 * i] = rec[kRecF64 * i], uv[2 * i + 1] = rec[kRecF64 * i + 1];
      if (idepth) idepth[i] = rec[kRecF64 * i + 2];
      if (variance) variance[i] = rec[kRecF64 * i + 3];
      if (relative_baseline) relative_baseline[i] = rec[kRecF64 * i + 4];
      const unsigned long long w = bytes[i];
      if (flags) flags[i] = static_cast<uint8_t>(w);
      if (type) type[i] = static_cast<uint8_t>(w >> 8);
      if (rgb) rgb[3 * i] = static_cast<uint8_t>(w >> 16), rgb[3 * i + 1] = static_cast<uint8_t>(w >> 24), rgb[3 * i + 2] = static_cast<uint8_t>(w >> 32);
    }
  });
}

int dsopp_hip_map_export(dsopp_hip_map *m, const dsopp_hip_map_export_options *options, int32_t n_ids, const int32_t *frame_ids, int64_t capacity,
                         double *xyz, uint8_t *rgb, uint8_t *type, double *relative_baseline, double *idepth_variance, int32_t *keyframe_index,
                         int32_t *record_index, int64_t *count, int32_t *per_keyframe_counts) {
  return guarded([&] {
    if (!m) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null map");
    dsopp_hip_map::checkExportOptions(options, n_ids, frame_ids, capacity);
    m->sr.use();
    hipStream_t st = m->sr.stream;
    const dsopp_hip_map::ExportPlan p = m->plan(*options, n_ids, frame_ids);
    // the outputs asked for, on the device: sized by what can be written, each at a multiple of 8 bytes
    const size_t cap = static_cast<size_t>(capacity < p.total ? capacity : p.total);
    const auto pad8 = [](size_t b) { return (b + 7) & ~static_cast<size_t>(7); };
    const size_t o_xyz = 0, o_rb = o_xyz + (xyz ? 24 * cap : 0), o_var = o_rb + (relative_baseline ? 8 * cap : 0),
                 o_kf = o_var + (idepth_variance ? 8 * cap : 0), o_rec = o_kf + (keyframe_index ? pad8(4 * cap) : 0),
                 o_rgb = o_rec + (record_index ? pad8(4 * cap) : 0), o_type = o_rgb + (rgb ? pad8(3 * cap) : 0), o_end = o_type + (type ? pad8(cap) : 0);
    dsopp_hip_map::ExportOutputs out;
    if (cap && o_end) {
      m->d_out.reserve(o_end, 0, st);
      uint8_t *base = m->d_out.ptr;
      if (xyz) out.xyz = reinterpret_cast<double *>(base + o_xyz);
      if (relative_baseline) out.relative_baseline = reinterpret_cast<double *>(base + o_rb);
      if (idepth_variance) out.idepth_variance = reinterpret_cast<double *>(base + o_var);
      if (keyframe_index) out.keyframe_index = reinterpret_cast<int *>(base + o_kf);
      if (record_index) out.record_index = reinterpret_cast<int *>(base + o_rec);
      if (rgb) out.rgb = base + o_rgb;
      if (type) out.type = base + o_type;
    }
    m->enqueue(*options, p, static_cast<int64_t>(cap), out, st);
    m->sr.sync();
    const long long total = m->countResult(p.n_kf, per_keyframe_counts);
    if (count) *count = total;
    const size_t kept = static_cast<size_t>(total) < cap ? static_cast<size_t>(total) : cap;
    if (kept) {
      const auto fetch = [&](void *host, const void *dev, size_t bytes) {
        if (host) HIP_CHECK(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, st));
      };
      fetch(xyz, out.xyz, 24 * kept);
      fetch(rgb, out.rgb, 3 * kept);
      fetch(type, out.type, kept);
      fetch(relative_baseline, out.relative_baseline, 8 * kept);
      fetch(idepth_variance, out.idepth_variance, 8 * kept);
      fetch(keyframe_index, out.keyframe_index, 4 * kept);
      fetch(record_index, out.record_index, 4 * kept);
      m->sr.sync();
    }
    if (total > capacity) fail(DSOPP_HIP_ERR_CAPACITY, "%lld points, capacity %lld", total, static_cast<long long>(capacity));
  });
}

int dsopp_hip_map_export_device(dsopp_hip_map *m, const dsopp_hip_map_export_options *options, int32_t n_ids, const int32_t *frame_ids, int64_t capacity,
                                void *xyz_dev, void *rgb_dev, void *type_dev, void *relative_baseline_dev, void *idepth_variance_dev,
                                void *keyframe_index_dev, void *record_index_dev, int64_t *count, int32_t *per_keyframe_counts) {
  return guarded([&] {
    if (!m) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null map");
    dsopp_hip_map::checkExportOptions(options, n_ids, frame_ids, capacity);
    if ((reinterpret_cast<uintptr_t>(rgb_dev) & 3) || (reinterpret_cast<uintptr_t>(keyframe_index_dev) & 3) || (reinterpret_cast<uintptr_t>(record_index_dev) & 3) ||
        (reinterpret_cast<uintptr_t>(xyz_dev) & 7) || (reinterpret_cast<uintptr_t>(relative_baseline_dev) & 7) || (reinterpret_cast<uintptr_t>(idepth_variance_dev) & 7))
      fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "device outputs must be aligned to their element (the colours to 4 bytes)");
    m->sr.use();
    const dsopp_hip_map::ExportPlan p = m->plan(*options, n_ids, frame_ids);
    dsopp_hip_map::ExportOutputs out;
    out.xyz = static_cast<double *>(xyz_dev), out.relative_baseline = static_cast<double *>(relative_baseline_dev);
    out.idepth_variance = static_cast<double *>(idepth_variance_dev);
    out.rgb = static_cast<uint8_t *>(rgb_dev), out.type = static_cast<uint8_t *>(type_dev);
    out.keyframe_index = static_cast<int *>(keyframe_index_dev), out.record_index = static_cast<int *>(record_index_dev);
    m->enqueue(*options, p, capacity, out, m->sr.stream);
    m->in_flight = p.n_chunks > 0;
    if (!count && !per_keyframe_counts) return;  // enqueued only
    m->settle();
    const long long total = m->countResult(p.n_kf, per_keyframe_counts);
    if (count) *count = total;
    if (total > capacity) fail(DSOPP_HIP_ERR_CAPACITY, "%lld points, capacity %lld", total, static_cast<long long>(capacity));
  });
}

}  // extern "C"
