// tl_seg.hpp -- what the segmentation kernels (tl_seg.hip) and their host side (tl_api_seg.hip) share: the control block,
// the device pointers of one call, and the launch sequence.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tl {

constexpr int kSegMaxRegions = 64;      // quadrant (4) x numSec (<= 16)
constexpr int kSegRings = 64;           // sensorModel (only 64 is supported)
constexpr int kSegSectors = kSegRings * 6;
constexpr int kSegMaxBounds = 4096;     // polarBounds entries (the shipped config needs ~390 for 120 m)
constexpr int kSegMaxSeeds = 1024;      // ground_seed_num
constexpr int kSegEdgePerSector = 20;   // extractFromSection's largestPickedNum bound

// sizes and state of one call, written by the kernels, read back once at the end
struct SegCtl {
  int n_kept, n_cur, n_ng, n_ground, n_obj, n_seg, n_clusters, n_edge, n_general;
  int polar_num, height, width, invalid;
  int reg_m[kSegMaxRegions], reg_g[kSegMaxRegions], reg_v[kSegMaxRegions];
  int ring_cnt[kSegRings], ring_off[kSegRings];
  double mean_split, min_pitch, max_pitch, min_polar, max_polar;
};

struct SegParams {
  int n;                 // input points
  int n_regions, num_sec, n_bounds;
  double sec_bounds[16];
  double near_th;        // near_dis^2
  double sensor_height, min_range, max_range, plane_dis;
  int max_iter, seed_num, ring_min, min_seg;
  double start_r, delta_r, delta_p, delta_a;
  double polar_seed;     // minPolar / maxPolar at the start of the frame: 5.0 on a context's first frame, 0.0 after
  int hash_mask;         // open-addressing table of voxel keys: capacity - 1 (a power of two >= 2 n)
};

struct SegBufs {
  const double* aos;     // input, n x 3
  SegCtl* ctl;
  int* ring;             // n: beam id per input point, -1 if filtered
  int* cur;              // current_scan (below the height split), input indices
  int* cur_reg;          // its region, -1 for none
  int* ng;               // non_ground_scan, input indices
  int* reg_mem;          // n_regions x n: region members (input indices, region order)
  unsigned char* reg_flag;   // n_regions x n: fit set / ground flags of the members
  int* reg_g;            // n_regions x n: ground output of each region
  int* reg_v;            // n_regions x n: vertical output of each region
  int* ground;           // n: ground_scan
  int* obj;              // n: object_scan
  double* pol_val;       // n x 3: polarCor (polar, pitch, azimuth)
  double* bounds;        // kSegMaxBounds
  int* vox;              // n x 4: polar, pitch, azimuth index, voxel key
  int* hkey;             // hash_mask + 1
  int* hval;             // hash_mask + 1: smallest object index in the voxel
  int* parent;           // n: union-find
  int* csize;            // n: component size at its root
  int* croot;            // n: root per point
  int* cl_root;          // kept clusters in rank order: root, first position, size
  int* cl_off;
  int* cl_size;
  int* seg_local;        // n: segmented, object-local indices
  int* seg_orig;         // n: segmented, input indices
  int* seg_label;        // n
  double* boxes;         // n_clusters x 6
  int* ring_list;        // n: segmented positions bucketed by ring
  double* cv;            // n: curvature per ring entry
  int* sorted;           // n: sector entries sorted ascending (curvature, entry)
  int* genbuf;           // n: general entries per sector
  unsigned char* picked; // n
  int* edge_sec;         // kSegSectors x 20: ring-local point ids
  int* sec_cnt;          // kSegSectors x 2: edge, general counts
  int* sec_base;         // kSegSectors: start of the sector's general entries in genbuf (ring offset + sector start)
  int* edge;             // n: edge_points, input indices
  int* general;          // n: general_points, input indices
};

// the whole stage, enqueued on `s`; returns the number of launches
int launch_segment(const SegParams& P, const SegBufs& B, hipStream_t s);

}  // namespace tl
