// tl_api_snapshot.hip -- C ABI of the closed map's snapshot (include/tloam_hip.h: tloam_closed_map_save_size, _save, _probe,
// _load; kernels in tl_snapshot.hip).
//
// The blob (format version 1, little-endian, every section a whole number of 64-bit words):
//   header      416 B   magic "TLCMSNP1", version, flags, bytes, checksum, n_kf, K, n_voxels, n_points, cloud_points, R, S,
//                       has_carve, has_surfels, has_clouds, sections (9), voxel, origin[3], then nine table entries
//                       (kind, 0, offset, bytes, checksum), kinds 1 .. 9 ascending; an absent section has 0 bytes
//   1 configs           the place, loop, closed map, carve and surfel configurations as their C structs, every reserve_* and
//                       reserved field 0
//   2 infos             tloam_closed_map_info (capacity_voxels 0), the carve's when carved, the surfels' when they exist
//   3 keyframes         frame [n_kf], stored pose [16 n_kf]                          (the host's PlaceState::kf)
//   4 poses             the build's poses [16 K]
//   5 database          ring keys [R n_kf], sector keys [S n_kf], descriptors [R S n_kf]   (the device's)
//   6 rows              key, N, Qx, Qy, Qz, each [n_voxels], in id order
//   7 misses            M [n_voxels], when carved
//   8 sums              the thirteen sums [13 n_voxels], when surfels exist
//   9 clouds            n [8 n_kf], then the clouds end to end in keyframe and slot order, AoS, with TLOAM_SNAPSHOT_CLOUDS
// NOT in it: normals and variances (k_surfel_solve gives them back from the sums), the localiser's records, table sizes and
// capacities, loop records, constraints, corrected graph poses, the localise and relocalise configurations.
//
// A save sizes the blob on the host, gathers sections 5 .. 9 into one device buffer with their checksums (one launch), brings
// them back in one copy and one wait, and writes the header and sections 1 .. 4 on the host.  It changes nothing in the context:
// its device buffer is its own.
// A load treats the blob as untrusted: the header, the table, sections 1 .. 4 and the clouds' counts are checked on the host;
// sections 5 .. 9 are uploaded into a staging buffer and checked there (k_snap_check); fresh stores are filled from the staging
// buffer and the slot table rebuilt from the keys is checked (k_snap_table); the normals and variances are solved from the loaded
// sums and their count compared with the saved info.  Only then is anything in the context replaced, by moves that cannot fail.
#include <math.h>

#include "tl_ctx.hpp"

using namespace tl;

namespace {

constexpr uint64_t kSnapMagic = 0x31504e534d434c54ull;   // "TLCMSNP1", little-endian
constexpr int kSections = 9;
enum Section { kConfigs = 1, kInfos, kKeyframes, kPoses, kDatabase, kRows, kMisses, kSums, kClouds };
const char* const kSectionName[kSections + 1] = {"header", "configs", "infos", "keyframes", "poses", "database",
                                                 "rows",   "misses",  "sums",  "clouds"};
constexpr int64_t kMaxKeyframes = (int64_t)1 << 30, kMaxVoxels = (int64_t)1 << 30, kMaxCloudPoints = (int64_t)1 << 40;

struct SnapEntry {
  uint32_t kind, reserved0;
  uint64_t offset, bytes, checksum;
};
struct SnapHeader {
  uint64_t magic;
  uint32_t version, flags;
  uint64_t bytes, checksum;
  int64_t n_kf, K, n_voxels, n_points, cloud_points;
  int32_t n_rings, n_sectors, has_carve, has_surfels, has_clouds, n_sections;
  double voxel, origin[3];
  SnapEntry sec[kSections];
};
static_assert(sizeof(SnapEntry) == 32 && sizeof(SnapHeader) == 416, "the header of format version 1");

struct SnapConfigs {
  tloam_place_config place;
  tloam_loop_config loop;
  tloam_closed_map_config cmap;
  tloam_closed_map_carve_config carve;
  tloam_closed_map_surfel_config surfel;
};
static_assert(sizeof(SnapConfigs) == 312, "the configs section of format version 1");
static_assert(sizeof(tloam_closed_map_info) == 64 && sizeof(tloam_closed_map_carve_info) == 64 &&
                  sizeof(tloam_closed_map_surfel_info) == 40,
              "the infos section of format version 1");

uint64_t mix64_host(uint64_t x) {   // tl_voxel.hpp mix64
  x ^= x >> 30; x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27; x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

// the checksum of `bytes` (a multiple of 8) at p, which need not be aligned
uint64_t checksum_host(const void* p, size_t bytes) {
  const unsigned char* b = (const unsigned char*)p;
  uint64_t sum = 0;
  for (size_t i = 0; i < bytes / 8; ++i) {
    uint64_t w;
    memcpy(&w, b + 8 * i, 8);
    sum += mix64_host(w + kSnapGolden * (uint64_t)(i + 1));
  }
  return sum;
}

uint64_t header_checksum(SnapHeader H) {
  H.checksum = 0;
  return checksum_host(&H, sizeof(H));
}

// the bytes of every section from the header's counts (which the caller has bounded)
void section_sizes(const SnapHeader& H, uint64_t size[kSections + 1]) {
  const uint64_t nk = (uint64_t)H.n_kf, K = (uint64_t)H.K, nv = (uint64_t)H.n_voxels, R = (uint64_t)H.n_rings,
                 S = (uint64_t)H.n_sectors, cp = (uint64_t)H.cloud_points;
  size[0] = sizeof(SnapHeader);
  size[kConfigs] = sizeof(SnapConfigs);
  size[kInfos] = sizeof(tloam_closed_map_info) + (H.has_carve ? sizeof(tloam_closed_map_carve_info) : 0) +
                 (H.has_surfels ? sizeof(tloam_closed_map_surfel_info) : 0);
  size[kKeyframes] = 8 * 17 * nk;
  size[kPoses] = 8 * 16 * K;
  size[kDatabase] = 8 * nk * (R + S + R * S);
  size[kRows] = 8 * 5 * nv;
  size[kMisses] = H.has_carve ? 8 * nv : 0;
  size[kSums] = H.has_surfels ? 8 * (uint64_t)kSurfelSums * nv : 0;
  size[kClouds] = H.has_clouds ? 8 * (8 * nk + 3 * cp) : 0;
}

// the table of a header whose counts are set: the sections end to end behind the header; returns the blob's bytes
uint64_t fill_table(SnapHeader* H) {
  uint64_t size[kSections + 1], at = sizeof(SnapHeader);
  section_sizes(*H, size);
  for (int k = 1; k <= kSections; ++k) {
    H->sec[k - 1] = SnapEntry{(uint32_t)k, 0u, at, size[k], 0ull};
    at += size[k];
  }
  H->n_sections = kSections;
  H->bytes = at;
  return at;
}

bool fail(std::string* err, const std::string& what) {
  if (err) *err = "closed map snapshot: " + what;
  return false;
}

// the header and the table of a blob of `bytes` bytes: *H when they hold
bool probe_header(const void* buf, size_t bytes, SnapHeader* H, std::string* err) {
  if (bytes < sizeof(SnapHeader)) return fail(err, "header: the blob is shorter than a header");
  memcpy(H, buf, sizeof(SnapHeader));
  if (H->magic != kSnapMagic) return fail(err, "header: wrong magic");
  if (H->version != TLOAM_SNAPSHOT_FORMAT_VERSION) return fail(err, "header: format version is not 1");
  if (H->checksum != header_checksum(*H)) return fail(err, "header: checksum");
  if (H->flags & ~(uint32_t)TLOAM_SNAPSHOT_CLOUDS) return fail(err, "header: unknown flag bits");
  if (H->n_sections != kSections) return fail(err, "header: section count");
  for (int32_t f : {H->has_carve, H->has_surfels, H->has_clouds})
    if (f != 0 && f != 1) return fail(err, "header: a has_* field is not 0 or 1");
  if (H->has_clouds != (int32_t)(H->flags & TLOAM_SNAPSHOT_CLOUDS)) return fail(err, "header: has_clouds is not the clouds flag");
  if (H->n_kf < 0 || H->n_kf > kMaxKeyframes) return fail(err, "header: n_keyframes_database out of range");
  if (H->K < 0 || H->K > H->n_kf) return fail(err, "header: K > n_kf");
  if (H->n_voxels < 0 || H->n_voxels > kMaxVoxels) return fail(err, "header: n_voxels > 2^30");
  if (H->n_points < 0 || H->n_points > (int64_t)kSnapMaxN) return fail(err, "header: n_points > 2^30");
  if (H->cloud_points < 0 || H->cloud_points > kMaxCloudPoints || (!H->has_clouds && H->cloud_points != 0))
    return fail(err, "header: cloud_points out of range");
  if (H->n_rings < 1 || H->n_rings > kPlaceMaxRings || H->n_sectors < 2 || H->n_sectors > kPlaceMaxSectors)
    return fail(err, "header: rings / sectors out of range");
  if (!(H->voxel > 0.0 && std::isfinite(H->voxel) && std::isfinite(H->origin[0]) && std::isfinite(H->origin[1]) &&
        std::isfinite(H->origin[2])))
    return fail(err, "header: voxel / origin");
  uint64_t size[kSections + 1], at = sizeof(SnapHeader);
  section_sizes(*H, size);
  for (int k = 1; k <= kSections; ++k) {
    const SnapEntry& E = H->sec[k - 1];
    const std::string name = kSectionName[k];
    if (E.kind != (uint32_t)k || E.reserved0 != 0) return fail(err, name + ": table entry kind");
    if (E.offset % 8 || E.bytes % 8) return fail(err, name + ": not 8-byte aligned");
    if (E.offset > bytes || E.bytes > bytes - E.offset) return fail(err, name + ": section past the end of the blob");
    if (E.offset < at) return fail(err, name + ": overlaps the section before it");
    if (E.offset != at) return fail(err, name + ": a gap before the section");
    if (E.bytes != size[k]) return fail(err, name + ": size is not what the counts ask for");
    at += E.bytes;
  }
  if (H->bytes != bytes || at != bytes) return fail(err, "header: bytes is not the blob's size");   // (after the table: a truncated blob names the section it cuts)
  return true;
}

void info_of(const SnapHeader& H, tloam_closed_map_snapshot_info* I) {
  memset(I, 0, sizeof(*I));
  I->format_version = (int32_t)H.version;
  I->flags = (int32_t)H.flags;
  I->n_keyframes_database = H.n_kf;
  I->n_keyframes_map = H.K;
  I->n_voxels = H.n_voxels;
  I->n_points = H.n_points;
  I->has_carve = H.has_carve; I->has_surfels = H.has_surfels; I->has_clouds = H.has_clouds;
  I->n_rings = H.n_rings; I->n_sectors = H.n_sectors;
  I->cloud_points = H.cloud_points;
  I->voxel = H.voxel;
  for (int a = 0; a < 3; ++a) I->origin[a] = H.origin[a];
  I->bytes = H.bytes;
}

// the header a save of this context writes, table and all but the checksums
int header_of(const tloam_ctx* c, int flags, SnapHeader* H) {
  if (!c || c->nranks > 1 || (flags & ~TLOAM_SNAPSHOT_CLOUDS)) return TLOAM_E_INVALID;
  const CmapState& M = c->cmap;
  const PlaceState& P = c->place;
  if (!M.built) return TLOAM_E_NOT_READY;
  memset(H, 0, sizeof(*H));
  H->magic = kSnapMagic;
  H->version = TLOAM_SNAPSHOT_FORMAT_VERSION;
  H->flags = (uint32_t)flags;
  H->n_kf = P.n_kf;
  H->K = (int64_t)(M.poses.size() / 16);
  H->n_voxels = M.info.n_voxels;
  H->n_points = M.info.n_points;
  H->n_rings = P.cfg.n_rings; H->n_sectors = P.cfg.n_sectors;
  H->has_carve = M.carved ? 1 : 0;
  H->has_surfels = M.surfeled ? 1 : 0;
  H->has_clouds = (flags & TLOAM_SNAPSHOT_CLOUDS) ? 1 : 0;
  if (H->has_clouds)
    for (const PlaceState::Keyframe& k : P.kf)
      for (int j = 0; j < 8; ++j) H->cloud_points += (int64_t)k.n[j];
  H->voxel = M.cfg.voxel;
  for (int a = 0; a < 3; ++a) H->origin[a] = M.cfg.origin[a];
  fill_table(H);
  return TLOAM_OK;
}

SnapConfigs configs_of(const tloam_ctx* c) {
  SnapConfigs G;
  G.place = c->place.cfg; G.loop = c->loop.cfg; G.cmap = c->cmap.cfg; G.carve = c->cmap.carve_cfg; G.surfel = c->cmap.surfel_cfg;
  G.place.reserved0 = 0; G.place.reserve_keyframes = 0;
  G.loop.reserved0 = 0; G.loop.reserve_points = 0; G.loop.coarse.reserved0 = 0;
  G.cmap.reserved0 = 0; G.cmap.reserve_voxels = 0;
  G.carve.reserved0 = 0;
  G.surfel.reserved0 = 0;
  return G;
}

SnapPiece piece(const void* src, void* dst, uint64_t words, uint64_t first, int section, int test = kSnapTestNone,
                const void* aux = nullptr, uint64_t aux_n = 0) {
  return SnapPiece{(const unsigned long long*)src, (unsigned long long*)dst, words, first, (const long long*)aux, aux_n, section, test};
}

// the device half of a save: sections 5 .. 9 gathered into `dev` (the blob from sec[kDatabase - 1].offset on), their checksums
// into H->sec, the bytes into `out`; one copy back, one wait
int save_device(tloam_ctx* c, SnapHeader* H, unsigned char* out) {
  const CmapState& M = c->cmap;
  const PlaceState& P = c->place;
  const uint64_t base = H->sec[kDatabase - 1].offset, words = (H->bytes - base) / 8;
  const uint64_t nk = (uint64_t)H->n_kf, nv = (uint64_t)H->n_voxels, R = (uint64_t)H->n_rings, S = (uint64_t)H->n_sectors;
  DBuf<unsigned long long> dev, ctl;   // the save's own, freed with it
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, dev.reserve(std::max<uint64_t>(words, 1))); HIPC(c, ctl.reserve(kSnapCtlWords));
  HIPC(c, hipMemsetAsync(ctl.p, 0, sizeof(unsigned long long) * kSnapCtlWords, c->stream));
  auto at = [&](int k) { return dev.p + (H->sec[k - 1].offset - base) / 8; };
  SnapPieces A;
  memset(&A, 0, sizeof(A));
  A.ctl = ctl.p;
  int& np = A.npieces;
  A.piece[np++] = piece(P.rkey.p, at(kDatabase), nk * R, 0, kDatabase);
  A.piece[np++] = piece(P.skey.p, at(kDatabase) + nk * R, nk * S, nk * R, kDatabase);
  A.piece[np++] = piece(P.desc.p, at(kDatabase) + nk * (R + S), nk * R * S, nk * (R + S), kDatabase);
  const void* const col[5] = {M.rows.key.p, M.rows.n.p, M.rows.qx.p, M.rows.qy.p, M.rows.qz.p};
  for (int j = 0; j < 5; ++j) A.piece[np++] = piece(col[j], at(kRows) + nv * j, nv, nv * j, kRows);
  if (H->has_carve) A.piece[np++] = piece(M.miss.p, at(kMisses), nv, 0, kMisses);
  if (H->has_surfels) A.piece[np++] = piece(M.surfel_sums.p, at(kSums), (uint64_t)kSurfelSums * nv, 0, kSums);
  std::vector<int64_t> counts;   // (alive until the wait below)
  if (H->has_clouds) {
    // the counts from the host's table, the clouds device to device: slot order, runs that lie end to end in the arena as one copy
    counts.resize(8 * nk);
    unsigned long long* const dst0 = at(kClouds) + 8 * nk;
    size_t done = 0, run_off = 0, run_n = 0;   // doubles
    auto flush = [&]() -> hipError_t {
      const hipError_t e = run_n ? hipMemcpyAsync(dst0 + done, P.arena.p + run_off, sizeof(double) * run_n, hipMemcpyDeviceToDevice, c->stream)
                                 : hipSuccess;
      done += run_n;
      run_n = 0;
      return e;
    };
    for (size_t k = 0; k < nk; ++k)
      for (int j = 0; j < 8; ++j) {
        const size_t n3 = 3 * P.kf[k].n[j];
        counts[8 * k + j] = (int64_t)P.kf[k].n[j];
        if (n3 == 0) continue;
        if (run_n && P.kf[k].off[j] == run_off + run_n) { run_n += n3; continue; }
        HIPC(c, flush());
        run_off = P.kf[k].off[j];
        run_n = n3;
      }
    HIPC(c, flush());
    if (nk) HIPC(c, hipMemcpyAsync(at(kClouds), counts.data(), sizeof(int64_t) * 8 * nk, hipMemcpyHostToDevice, c->stream));
    A.piece[np++] = piece(at(kClouds), nullptr, H->sec[kClouds - 1].bytes / 8, 0, kClouds);
  }
  launch_snap_pack(A, c->stream);
  HIPC(c, hipGetLastError());
  unsigned long long sums[kSnapCtlWords];
  if (words) HIPC(c, hipMemcpyAsync(out + base, dev.p, 8 * words, hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipMemcpyAsync(sums, ctl.p, sizeof(sums), hipMemcpyDeviceToHost, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  for (int k = kDatabase; k <= kClouds; ++k) H->sec[k - 1].checksum = sums[k];
  return TLOAM_OK;
}

// ---- load ----
// sections 1 .. 4 and the clouds' counts of a blob whose header holds, out of the blob and checked
struct HostSections {
  SnapConfigs cfg;
  tloam_closed_map_info info;
  tloam_closed_map_carve_info carve_info;
  tloam_closed_map_surfel_info surfel_info;
  std::vector<int64_t> frame;
  std::vector<double> kf_pose, poses;
  std::vector<int64_t> cloud_n;   // [8 n_kf] (empty without clouds)
};

bool all_finite(const std::vector<double>& v) {
  for (double x : v)
    if (!std::isfinite(x)) return false;
  return true;
}

bool host_sections(const unsigned char* b, const SnapHeader& H, HostSections* X, std::string* err) {
  for (int k = kConfigs; k <= kPoses; ++k)
    if (checksum_host(b + H.sec[k - 1].offset, H.sec[k - 1].bytes) != H.sec[k - 1].checksum)
      return fail(err, std::string(kSectionName[k]) + ": checksum");
  const size_t nk = (size_t)H.n_kf, K = (size_t)H.K;
  // configs
  memcpy(&X->cfg, b + H.sec[kConfigs - 1].offset, sizeof(SnapConfigs));
  const SnapConfigs& G = X->cfg;
  if (!place_config_valid(G.place) || G.place.enabled != 1) return fail(err, "configs: place configuration (place_config_ok, enabled)");
  if (!loop_config_valid(G.loop) || G.loop.enabled != 1) return fail(err, "configs: loop configuration (loop_config_ok, enabled)");
  if (!cmap_config_valid(G.cmap)) return fail(err, "configs: closed map configuration (cmap_config_ok)");
  if (!carve_config_valid(G.carve)) return fail(err, "configs: carve configuration (carve_config_ok)");
  if (G.surfel.min_points < 3) return fail(err, "configs: surfel configuration (min_points < 3)");
  if (G.place.reserved0 || G.place.reserve_keyframes || G.loop.reserved0 || G.loop.reserve_points || G.loop.coarse.reserved0 ||
      G.cmap.reserved0 || G.cmap.reserve_voxels || G.carve.reserved0 || G.surfel.reserved0)
    return fail(err, "configs: a reserve field is not 0");
  if (G.place.n_rings != H.n_rings || G.place.n_sectors != H.n_sectors || memcmp(&G.cmap.voxel, &H.voxel, sizeof(double)) != 0 ||
      memcmp(G.cmap.origin, H.origin, sizeof(H.origin)) != 0)
    return fail(err, "configs: rings, sectors, voxel or origin are not the header's");
  // infos
  const unsigned char* p = b + H.sec[kInfos - 1].offset;
  memcpy(&X->info, p, sizeof(X->info));
  p += sizeof(X->info);
  memset(&X->carve_info, 0, sizeof(X->carve_info));
  memset(&X->surfel_info, 0, sizeof(X->surfel_info));
  if (H.has_carve) { memcpy(&X->carve_info, p, sizeof(X->carve_info)); p += sizeof(X->carve_info); }
  if (H.has_surfels) memcpy(&X->surfel_info, p, sizeof(X->surfel_info));
  const tloam_closed_map_info& I = X->info;
  if (I.n_keyframes != H.K || I.n_voxels != H.n_voxels || I.n_points != H.n_points || I.capacity_voxels != 0)
    return fail(err, "infos: the closed map's counts are not the header's");
  if (I.added_keyframes < 0 || I.empty_keyframes < 0 || I.overflow_keyframes < 0 ||
      I.added_keyframes + I.empty_keyframes + I.overflow_keyframes != H.K || I.pose_source < TLOAM_CLOSED_MAP_POSES_STORED ||
      I.pose_source > TLOAM_CLOSED_MAP_POSES_CALLER)
    return fail(err, "infos: the closed map's keyframe counts or pose source");
  if (H.has_carve && X->carve_info.n_keyframes != H.K) return fail(err, "infos: the carve's keyframes are not the header's K");
  if (H.has_surfels && (X->surfel_info.n_keyframes != H.K || X->surfel_info.solved_voxels < 0 ||
                        X->surfel_info.solved_voxels > H.n_voxels))
    return fail(err, "infos: the surfels' keyframes or solved voxels");
  // keyframes and poses
  X->frame.resize(nk); X->kf_pose.resize(16 * nk); X->poses.resize(16 * K);
  p = b + H.sec[kKeyframes - 1].offset;
  if (nk) { memcpy(X->frame.data(), p, 8 * nk); memcpy(X->kf_pose.data(), p + 8 * nk, 128 * nk); }
  if (K) memcpy(X->poses.data(), b + H.sec[kPoses - 1].offset, 128 * K);
  if (!all_finite(X->kf_pose)) return fail(err, "keyframes: a stored pose is not finite");
  if (!all_finite(X->poses)) return fail(err, "poses: a pose of the build is not finite");
  for (size_t k = 0; k < K; ++k) {
    Pose unused;
    if (!pose_from_matrix(X->poses.data() + 16 * k, &unused)) return fail(err, "poses: a pose of the build is not rigid (pose_from_matrix)");
  }
  // the clouds' counts
  if (H.has_clouds) {
    X->cloud_n.resize(8 * nk);
    if (nk) memcpy(X->cloud_n.data(), b + H.sec[kClouds - 1].offset, 64 * nk);
    int64_t all = 0;
    for (int64_t n : X->cloud_n) {
      if (n < 0 || n > (int64_t)kMaxPoints) return fail(err, "clouds: a cloud's count out of range");
      all += n;
      if (all > H.cloud_points) break;
    }
    if (all != H.cloud_points) return fail(err, "clouds: the counts do not sum to the section's points");
  }
  return true;
}

// the fresh state of a load, the loader's own until it is moved into the context
struct Fresh {
  PlaceState place;
  VoxelRowStore rows;
  DBuf<unsigned long long> miss, sums, surfel_ctl;
  DBuf<double> nrm, ev;
  DBuf<int> over;
};

int refuse(tloam_ctx* c, const std::string& what) {
  c->last_error = "closed map snapshot: " + what;
  return TLOAM_E_INVALID;
}

int load_body(tloam_ctx* c, const unsigned char* b, const SnapHeader& H, const HostSections& X, Fresh* F) {
  const uint64_t base = H.sec[kDatabase - 1].offset, words = (H.bytes - base) / 8;
  const uint64_t nk = (uint64_t)H.n_kf, nv = (uint64_t)H.n_voxels, R = (uint64_t)H.n_rings, S = (uint64_t)H.n_sectors,
                 K = (uint64_t)H.K, cp = (uint64_t)H.cloud_points;
  const hipMemcpyKind H2D = hipMemcpyHostToDevice, D2D = hipMemcpyDeviceToDevice, D2H = hipMemcpyDeviceToHost;
  // 1. the device-born sections into a staging buffer, summed and tested there
  DBuf<unsigned long long> stage, ctl;
  HIPC(c, stage.reserve(std::max<uint64_t>(words, 1))); HIPC(c, ctl.reserve(kSnapCtlWords));
  HIPC(c, hipMemsetAsync(ctl.p, 0, sizeof(unsigned long long) * kSnapCtlWords, c->stream));
  if (words) HIPC(c, hipMemcpyAsync(stage.p, b + base, 8 * words, H2D, c->stream));
  auto at = [&](int k) { return stage.p + (H.sec[k - 1].offset - base) / 8; };
  SnapPieces A;
  memset(&A, 0, sizeof(A));
  A.ctl = ctl.p;
  int& np = A.npieces;
  A.piece[np++] = piece(at(kDatabase), nullptr, nk * (R + S + R * S), 0, kDatabase, kSnapTestFinite);
  A.piece[np++] = piece(at(kRows), nullptr, nv, 0, kRows, kSnapTestKey);
  A.piece[np++] = piece(at(kRows) + nv, nullptr, nv, nv, kRows, kSnapTestN);
  A.piece[np++] = piece(at(kRows) + 2 * nv, nullptr, 3 * nv, 2 * nv, kRows, kSnapTestQ, at(kRows) + nv, nv);
  if (H.has_carve) A.piece[np++] = piece(at(kMisses), nullptr, nv, 0, kMisses, kSnapTestMiss);
  if (H.has_surfels) A.piece[np++] = piece(at(kSums), nullptr, (uint64_t)kSurfelSums * nv, 0, kSums, kSnapTestSums);
  if (H.has_clouds) A.piece[np++] = piece(at(kClouds), nullptr, H.sec[kClouds - 1].bytes / 8, 0, kClouds);
  launch_snap_check(A, c->stream);
  HIPC(c, hipGetLastError());
  unsigned long long w[kSnapCtlWords];
  HIPC(c, hipMemcpyAsync(w, ctl.p, sizeof(w), D2H, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  for (int k = kDatabase; k <= kClouds; ++k)
    if (w[k] != H.sec[k - 1].checksum) return refuse(c, std::string(kSectionName[k]) + ": checksum");
  if (w[kSnapBadFinite]) return refuse(c, "database: a key or descriptor value is not finite");
  if (w[kSnapBadKey]) return refuse(c, "rows: a key with an axis field of 0 or bit 63 set");
  if (w[kSnapBadN]) return refuse(c, "rows: N outside [1, 2^30]");
  if (w[kSnapBadQ]) return refuse(c, "rows: Q outside [0, N * 2^24]");
  if (w[kSnapSumN] != (unsigned long long)H.n_points) return refuse(c, "rows: the sum of N is not n_points");
  if (w[kSnapBadMiss]) return refuse(c, "misses: M < 0");
  if (w[kSnapBadSums]) return refuse(c, "sums: Ns, Sxx, Syy or Szz < 0");
  // 2. fresh stores filled from the staging buffer; the slot table rebuilt from the keys and checked
  PlaceState& P = F->place;
  P.cfg = X.cfg.place;
  const size_t kcap = std::max<size_t>((size_t)nk, place_default_reserve());
  HIPC(c, P.bins.reserve(R * S));
  HIPC(c, hipMemsetAsync(P.bins.p, 0, sizeof(unsigned long long) * P.bins.cap, c->stream));
  HIPC(c, P.ctl.reserve(1));
  HIPC(c, hipMemsetAsync(P.ctl.p, 0, sizeof(unsigned long long), c->stream));
  HIPC(c, P.cand.reserve(kPlaceMaxCandidates));
  HIPC(c, P.desc.reserve(kcap * R * S)); HIPC(c, P.rkey.reserve(kcap * R)); HIPC(c, P.skey.reserve(kcap * S));
  HIPC(c, P.pose.reserve(kcap * 16)); HIPC(c, P.frame.reserve(kcap)); HIPC(c, P.loops.reserve(kcap));
  HIPC(c, P.kdist.reserve(kcap)); HIPC(c, P.taken.reserve(kcap));
  P.cap = kcap;
  if (nk) {
    HIPC(c, hipMemcpyAsync(P.rkey.p, at(kDatabase), 8 * nk * R, D2D, c->stream));
    HIPC(c, hipMemcpyAsync(P.skey.p, at(kDatabase) + nk * R, 8 * nk * S, D2D, c->stream));
    HIPC(c, hipMemcpyAsync(P.desc.p, at(kDatabase) + nk * (R + S), 8 * nk * R * S, D2D, c->stream));
    HIPC(c, hipMemcpyAsync(P.frame.p, X.frame.data(), 8 * nk, H2D, c->stream));
    HIPC(c, hipMemcpyAsync(P.pose.p, X.kf_pose.data(), 128 * nk, H2D, c->stream));
  }
  HIPC(c, P.arena.reserve(std::max<size_t>(3 * (size_t)cp, 3 * ((size_t)1 << 20))));   // (tloam_loop_configure's default room)
  if (cp) HIPC(c, hipMemcpyAsync(P.arena.p, at(kClouds) + 8 * nk, 24 * cp, D2D, c->stream));
  P.kf.resize((size_t)nk);
  for (size_t k = 0; k < nk; ++k) {
    PlaceState::Keyframe& Kf = P.kf[k];
    memset(&Kf, 0, sizeof(Kf));
    Kf.frame = X.frame[k];
    memcpy(Kf.pose, &X.kf_pose[16 * k], sizeof(Kf.pose));
    for (int j = 0; j < 8; ++j) {
      Kf.off[j] = P.arena_used;
      Kf.n[j] = H.has_clouds ? (size_t)X.cloud_n[8 * k + j] : 0;
      P.arena_used += 3 * Kf.n[j];
    }
  }
  P.n_kf = (int64_t)nk;
  if (nk) {
    P.last_kf_frame = X.frame[nk - 1];
    memcpy(P.last_pose, &X.kf_pose[16 * (nk - 1)], sizeof(P.last_pose));
  }
  VoxelRowStore& Rw = F->rows;
  const size_t cap = std::max<size_t>((size_t)nv, cmap_default_reserve());
  size_t tsize = 1024;
  while (tsize < 2 * cap) tsize <<= 1;
  HIPC(c, Rw.key.reserve(cap));
  for (DBuf<long long>* a : {&Rw.n, &Rw.qx, &Rw.qy, &Rw.qz}) HIPC(c, a->reserve(cap));
  HIPC(c, Rw.tab.reserve(tsize));
  Rw.cap = cap;
  Rw.tmask = tsize - 1;
  if (nv) {
    void* const col[5] = {Rw.key.p, Rw.n.p, Rw.qx.p, Rw.qy.p, Rw.qz.p};
    for (int j = 0; j < 5; ++j) HIPC(c, hipMemcpyAsync(col[j], at(kRows) + nv * j, 8 * nv, D2D, c->stream));
  }
  HIPC(c, hipMemsetAsync(Rw.tab.p, 0xff, sizeof(int) * tsize, c->stream));
  launch_snap_table(Rw.table(), (size_t)nv, ctl.p, c->stream);
  HIPC(c, hipGetLastError());
  if (H.has_carve) {
    HIPC(c, F->miss.reserve(std::max<size_t>((size_t)nv, 1)));
    if (nv) HIPC(c, hipMemcpyAsync(F->miss.p, at(kMisses), 8 * nv, D2D, c->stream));
  }
  if (H.has_surfels) {
    // 3. the normals and the variances: k_surfel_solve alone, on the loaded sums
    HIPC(c, F->sums.reserve((size_t)kSurfelSums * cap)); HIPC(c, F->nrm.reserve(3 * cap)); HIPC(c, F->ev.reserve(3 * cap));
    HIPC(c, F->over.reserve(std::max<size_t>((size_t)K, 1))); HIPC(c, F->surfel_ctl.reserve(8));
    if (nv) HIPC(c, hipMemcpyAsync(F->sums.p, at(kSums), 8 * (size_t)kSurfelSums * nv, D2D, c->stream));
    HIPC(c, hipMemsetAsync(F->surfel_ctl.p, 0, sizeof(unsigned long long) * 8, c->stream));
    SurfelWork W;
    memset(&W, 0, sizeof(W));
    W.grid.voxel = X.cfg.cmap.voxel;   // (all k_surfel_solve reads of the map)
    W.grid.nv = (long long)nv;
    W.min_points = X.cfg.surfel.min_points;
    W.sums = F->sums.p; W.normal = F->nrm.p; W.eval = F->ev.p; W.ctl = F->surfel_ctl.p;
    launch_surfel_solve(W, c->stream);
    HIPC(c, hipGetLastError());
  }
  unsigned long long solved[3] = {0, 0, 0};
  HIPC(c, hipMemcpyAsync(w, ctl.p, sizeof(w), D2H, c->stream));
  if (H.has_surfels) HIPC(c, hipMemcpyAsync(solved, F->surfel_ctl.p, sizeof(solved), D2H, c->stream));
  HIPC(c, hipStreamSynchronize(c->stream));
  if (w[kSnapBadFind]) return refuse(c, "rows: a key is held by two voxels (the rebuilt table does not find every id)");
  if (H.has_surfels && solved[2] != (unsigned long long)X.surfel_info.solved_voxels)
    return refuse(c, "infos: the surfels' solved voxels are not those of the sums");
  return TLOAM_OK;
}

}  // namespace

extern "C" {

int tloam_closed_map_save_size(tloam_ctx* c, int flags, size_t* bytes) {
  if (!bytes) return TLOAM_E_INVALID;
  SnapHeader H;
  const int rc = header_of(c, flags, &H);
  if (rc != TLOAM_OK) return rc;
  *bytes = (size_t)H.bytes;
  return TLOAM_OK;
}

int tloam_closed_map_save(tloam_ctx* c, int flags, void* buf, size_t capacity, size_t* written) {
  if (written) *written = 0;
  if (!written) return TLOAM_E_INVALID;
  SnapHeader H;
  int rc = header_of(c, flags, &H);
  if (rc != TLOAM_OK) return rc;
  *written = (size_t)H.bytes;
  if (!buf || capacity < H.bytes) return TLOAM_E_INVALID;
  unsigned char* const out = (unsigned char*)buf;
  rc = save_device(c, &H, out);
  if (rc != TLOAM_OK) {
    (void)hipStreamSynchronize(c->stream);   // (nothing of the save is in flight when its buffer goes)
    return rc;
  }
  const CmapState& M = c->cmap;
  const PlaceState& P = c->place;
  const SnapConfigs G = configs_of(c);
  memcpy(out + H.sec[kConfigs - 1].offset, &G, sizeof(G));
  unsigned char* p = out + H.sec[kInfos - 1].offset;
  tloam_closed_map_info I = M.info;
  I.capacity_voxels = 0;
  memcpy(p, &I, sizeof(I));
  p += sizeof(I);
  if (M.carved) { memcpy(p, &M.carve_info, sizeof(M.carve_info)); p += sizeof(M.carve_info); }
  if (M.surfeled) memcpy(p, &M.surfel_info, sizeof(M.surfel_info));
  p = out + H.sec[kKeyframes - 1].offset;
  const size_t nk = (size_t)H.n_kf;
  for (size_t k = 0; k < nk; ++k) {
    memcpy(p + 8 * k, &P.kf[k].frame, 8);
    memcpy(p + 8 * nk + 128 * k, P.kf[k].pose, 128);
  }
  if (!M.poses.empty()) memcpy(out + H.sec[kPoses - 1].offset, M.poses.data(), sizeof(double) * M.poses.size());
  for (int k = kConfigs; k <= kPoses; ++k) H.sec[k - 1].checksum = checksum_host(out + H.sec[k - 1].offset, H.sec[k - 1].bytes);
  H.checksum = header_checksum(H);
  memcpy(out, &H, sizeof(H));
  return TLOAM_OK;
}

int tloam_closed_map_probe(const void* buf, size_t bytes, tloam_closed_map_snapshot_info* info) {
  if (!buf || !info) return TLOAM_E_INVALID;
  SnapHeader H;
  if (!probe_header(buf, bytes, &H, nullptr)) return TLOAM_E_INVALID;
  info_of(H, info);
  return TLOAM_OK;
}

int tloam_closed_map_load(tloam_ctx* c, const void* buf, size_t bytes, tloam_closed_map_snapshot_info* info) {
  if (!c || c->nranks > 1) return TLOAM_E_INVALID;
  if (!buf) return refuse(c, "header: no blob");
  SnapHeader H;
  HostSections X;
  if (!probe_header(buf, bytes, &H, &c->last_error)) return TLOAM_E_INVALID;
  if (!host_sections((const unsigned char*)buf, H, &X, &c->last_error)) return TLOAM_E_INVALID;
  HIPC(c, hipSetDevice(c->device));
  HIPC(c, hipStreamSynchronize(c->stream));   // (as tloam_place_configure: what is in flight may read what is replaced below)
  Fresh F;
  const int rc = load_body(c, (const unsigned char*)buf, H, X, &F);
  if (rc != TLOAM_OK) {
    (void)hipStreamSynchronize(c->stream);   // (nothing of the load is in flight when its storage goes)
    return rc;
  }
  // from here on nothing fails: the run's place / loop / graph / closed-map state is replaced
  c->place = std::move(F.place);
  c->loop.clear();
  c->loop.cfg = X.cfg.loop;
  c->loop.cfg_set = true;
  c->graph.drop();
  CmapState& M = c->cmap;
  M.drop();
  M.cfg = X.cfg.cmap;
  M.rows = std::move(F.rows);
  M.info = X.info;
  M.poses = X.poses;
  M.built = true;
  M.detached = !H.has_clouds;
  M.carve_cfg = X.cfg.carve;
  if (H.has_carve) {
    M.miss = std::move(F.miss);
    M.carve_info = X.carve_info;
    M.carved = true;
  }
  M.surfel_cfg = X.cfg.surfel;
  if (H.has_surfels) {
    M.surfel_sums = std::move(F.sums); M.surfel_nrm = std::move(F.nrm); M.surfel_ev = std::move(F.ev);
    M.surfel_over = std::move(F.over); M.surfel_ctl = std::move(F.surfel_ctl);
    M.surfel_info = X.surfel_info;
    M.surfeled = true;
  }
  if (info) info_of(H, info);
  return TLOAM_OK;
}

}  // extern "C"
