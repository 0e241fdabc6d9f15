/*
 * bev_internal.h — shared between the HIP kernels (bev_kernels.hip) and the
 * C-ABI / context code (bev_capi*.hip).  Not installed; the public boundary is
 * include/bev_mi355x.h.
 */
#ifndef BEV_INTERNAL_H
#define BEV_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/bev_mi355x.h"
#include "bev_exact.h"

namespace bevk {

constexpr int kGatherThreads = 256;
constexpr int kSlotsPerThread = 4;
constexpr int kTile = kGatherThreads * kSlotsPerThread; /* slots per workgroup of the gather kernel */
constexpr int kMaxTiles = 1024;   /* => at most 2^20 slots per frame (bev_create checks) */
constexpr int kStripThreads = 256;              /* column-walk workgroup: 236 columns + 2 halo columns each side = 240 virtual columns */
constexpr int kStripCols = 236;                 /* (256 input positions cover them with 16 to spare: the in-place source's window, one per thread) */
constexpr int kStripVirt = kStripCols + 4;
constexpr int kSeg = 256;                       /* capacity of one candidate segment = one (row, strip) */
constexpr int kMaxSegs = 1024;                  /* (G + 1) * strips must not exceed this (bev_create checks) */
constexpr int kSumWaves = 4;      /* waves of the per-frame cell-sum workgroup: the size of a column-walk workgroup */
constexpr int kSumThreads = kSumWaves * 64;
/* ONE workgroup shape for every kernel of the hot path — 256 threads, at most a quarter of a CU's LDS (32 of its 128
 * allocation granules of 1,280 bytes) and of its registers (128 per lane) — so that the stages of different sub-batches can
 * be workgroups of ONE launch (k_stage) and any of them fits wherever another has retired.  (Rounds 3-5 ran the resolve and
 * the rasters as 512-thread workgroups, the rasters with 50 KB of LDS: beside the column walk they started only where two
 * walk workgroups of one CU had retired together.) */
constexpr int kStageThreads = 256;
constexpr int kSlotLdsBytes = 32 * 1280;
constexpr int kResolveThreads = kStageThreads;
constexpr int kResolveParts = 4;  /* code lists per frame written by k_ground_resolve (a contiguous quarter of the segments each) */
/* workgroups per frame in k_ground_resolve, kResolveParts / kResolveWgs consecutive parts each: a workgroup's tables
 * (3,750 averages, their neighbour minima, edge bins, band table) cost as much as a part's candidates */
#ifndef BEV_RESOLVE_WGS
#define BEV_RESOLVE_WGS 2
#endif
constexpr int kResolveWgs = BEV_RESOLVE_WGS;
static_assert(kResolveParts % kResolveWgs == 0, "whole parts per workgroup");
constexpr int kRasterThreads = kStageThreads;
constexpr int kRasterLdsCap = kSlotLdsBytes; /* a raster band's two planes (+ its list prefix) */
constexpr int kRasterFineDiv = bevx::kBandFineDiv; /* (2) the middle bands of the image are cut this many times finer (see fill_geometry) */
constexpr int kRasterSplit = 8;   /* fewest x-bands per frame in the raster kernel (see raster_bands_for) */
constexpr int kMaxBands = bevx::kBandMax; /* (64) coarse + fine raster bands (see RasterParams) */
constexpr int kMaxStrips = 280;   /* ceil(65535 / kStripCols) rounded up */
/* Entries of one (emitter, band) code list.  Measured fill (scripts/list_fill.py: which capacities overflow on the
 * synthetic layouts): HDL_64E sweeps stay under 2,048 codes per list, OS1_64 frames under 3,072 — of the 15,104 slots a
 * strip has (the walk drops repeats of a code before they are listed); sized for the worst case the lists were 21.6 MB
 * per frame and workspace set, now 3.0 MB.  A writer whose list is full keeps counting and overwrites the list's
 * last entry; k_bev_raster sees the count and computes that band of the frame from the ordered cloud instead (it reads
 * all S slots: slow, correct, and only for clouds piled up in one band).  BEV_CODE_CAP (environment of bev_create)
 * overrides the size: the tests run with tiny lists. */
constexpr int kCodeListCap = 4096;
constexpr int kCtxTabWords = bevx::kGridRows + bevx::kGridCols + 512 / 4; /* BatchPtrs::ctx_tab */

/* per-frame launch metadata, copied H2D once per sub-batch */
struct FrameDesc {
    uint64_t in_offset; /* element offset of the frame's points in d_pts */
    uint32_t n_pts;
    uint32_t _pad;
};

/* How a frame's points reach their slots (getOrderedCloud, BatchMultiBevGen.cpp:94-117), decided per frame on the device:
 *   kFrameGeneral  any input: order scan over all points (winner table), the walk gathers through it;
 *   kFrameStream   the input's first T points are in strictly ascending slot order (a sweep written row by row, the
 *                  usual output of a selector): the walk reads them in place, row by row, and only the tail [T, n)
 *                  goes through the order scan; the walk VERIFIES the order of everything it consumes and counts it;
 *   kFrameRedo     a stream / structured frame whose verification failed: done again the general way (results never
 *                  depend on what k_probe guessed);
 *   kFrameStructured  the input IS a structured cloud of S records, what the KITTI selector writes
 *                  (KittiPointCloudSelect.cpp:206-207,240): record i is the point of slot i or an all-zero record.  The
 *                  scatter of getOrderedCloud is then the identity on every slot but slot 0, where every all-zero
 *                  record lands (row = col = 0): slot 0 ends up all-zero iff a record after the first is all-zero.  The
 *                  walk reads the records in place, once, coalesced, checks every one of them, and learns on the way
 *                  whether an all-zero record exists — which k_probe had to guess from its samples (the guess decides
 *                  slot 0 before the walk has seen the frame; a wrong guess is a failed frame);
 *   kFrameColMajor the input is S returns in firing order, the PLAIN sweep (BASELINE config 3): position k holds beam
 *                  k % N of firing k / N, its column is the firing's number plus 0 .. kPlainDisp (or out of range:
 *                  dropped).  The walk fetches a strip's firings band by band (two rows of a firing are one 64-byte
 *                  sector), settles the last writer of every slot in an LDS index row and checks every record it fetches;
 *   kFrameColMajorGen  ... what the MulRan selector writes for real sweeps (MulranPointCloudSelect.cpp:112-130): any start
 *                  azimuth, either direction, a base column per row (staggered beams) + 0 .. kColMaxDisp, no-return
 *                  records in column 0 (see the constants below; BatchPtrs::cm_par / cm_sync are this mode's alone). */
enum : uint32_t { kFrameGeneral = 0, kFrameStream = 1, kFrameRedo = 2, kFrameStructured = 3, kFrameColMajor = 4, kFrameColMajorGen = 5 };
__host__ __device__ inline bool frame_read_in_place(uint32_t mode) { return mode == kFrameStream || mode == kFrameStructured || mode == kFrameColMajor || mode == kFrameColMajorGen; }
struct FrameInfo {
    uint32_t T;        /* length of the prefix taken for sorted (structured: S) */
    uint32_t mode;
    uint32_t consumed; /* prefix points the stream walk has found in their own (row, strip) window (structured: records checked) */
    uint32_t failed;   /* bit 0: a consumed point was not above its predecessor, or could not be checked (structured: a
                        * record is neither its slot's point nor all-zero); structured frames also: bit 1: the walk saw an
                        * all-zero record after the first, bit 2: k_probe guessed that there is one */
};
constexpr uint32_t kInfoFailed = 1u, kInfoZeroSeen = 2u, kInfoZeroGuess = 4u;
constexpr uint32_t kInfoCmStray = 8u; /* firing-order frames whose strips do not talk: a strip other than 0 owns a no-return record: k_verdict checks that it would not have won column 0 */
constexpr uint32_t kInfoCmUsed = 16u; /* (a bit of its own: round 5 shared kInfoZeroSeen's, told apart by the frame's mode) firing-order frames: a wrap-around halo fell back on column 0 somewhere: k_verdict compares what it took with what strip 0 put there */
/* k_probe looks at every 63rd point of a frame (odd: no resonance with firing orders of 2^k beams) — at every 127th of a DENSE
 * sweep (at least nine tenths as many points as slots, and not exactly S records: those may be structured clouds or firing
 * orders, whose analysis wants its samples): the position of a slot between two samples is interpolated, its error grows with
 * the root of (stride x share of dropped returns), and the walk's windows have a dozen positions of slack — a sweep that
 * keeps 60 % of its returns fails its checks at 127 (tests/test_gpu_stream.py) and is fine at 63; the graded sweeps (98 %)
 * are fine at either, and the probe's samples are bytes: +1.8 % frames/s on the same box */
constexpr int kProbeStride = 63, kProbeStrideDense = 127;
constexpr int kMaxSamples = 4096;   /* => sorted frames of up to 258 k points are read in place (k_probe keeps their samples in LDS, a quarter of a CU's); longer ones go the general way */
constexpr int kStreamMinPrefix = 2048;
constexpr int kTailCap = 64;         /* tail points (those after the sorted prefix) a (row, strip) can list; more: general way */
constexpr int kTailMax = 16384;     /* ... a frame can have */
constexpr int kTailBuckets = 2048;  /* (row, strip) pairs of a frame that k_probe can count in LDS */
/* kFrameColMajor (round 5: any start azimuth, either direction of rotation, staggered beams, no-return records): with
 * u = +-firing mod H (the sweep's direction) a return of row r has column (u + B[r] + 0 .. kColMaxDisp) mod H, B[r] the
 * row's base (start azimuth + the beam's azimuth offset), or is out of range (>= H: dropped), or sits in column 0 whatever
 * its firing (a no-return record: x = y = 0 -> atan2(0, 0) = 0, MulranPointCloudSelect.cpp:123-125). */
constexpr int kPlainDisp = 8;        /* the PLAIN sweep (kFrameColMajor): column = firing + 0 .. kPlainDisp, or >= H (k_probe's test and k_walk<kSrcColMajor>'s check) */
constexpr int kColMaxDisp = 12;      /* (a row's displacements may spread over 8 columns and still leave k_probe, which sees every 63rd record, two columns of slack on either side) */
constexpr int kCmSpread = 18;        /* the rows' bases lie within this many columns of each other (an OS1-64's four laser columns: +-9) */
constexpr int kCmProbeDisp = kColMaxDisp; /* spread of a row's SAMPLED displacements that k_probe accepts; what is left of kColMaxDisp is put half below, half above them, for the records it did not see */
constexpr int kCmExt = 16;           /* firings behind the 256 threads' that a strip fetches as well: 272 >= 240 columns + kColMaxDisp + kCmSpread */
constexpr int kCmMaxRows = 128;      /* sensors with more rows go the general way */
constexpr int kCmMaxSamples = 4096;  /* k_probe keeps this many samples (and their successors) for the analysis: frames of up to 258 k records */
constexpr int kCmParWords = 4 + kCmMaxRows; /* per frame: direction (+1 / -1 as int), the largest base (mod H), the rows' bases, how far apart the bases lie, whether a sample was a no-return record */
constexpr uint32_t kCmUsedBit = 0x80000000u;
constexpr int kCmMaxStrips = 16;     /* strips other than 0 tell strip 0 about their no-return records, two words per band of two rows each: frames of more strips go the general way */
constexpr int kCmPubWords = (kCmMaxRows / 2) * kCmMaxStrips * 2; /* BatchPtrs::cm_sync per frame: [band][strip][2] reports, then [row] what strip 0 put into column 0, then [row] what a wrap-around halo took for it */
constexpr int kCmSyncWords = kCmPubWords + 3 * kCmMaxRows; /* ... then [row] the last no-return firing + 1 that a strip other than 0 owns, for frames whose strips do not talk (k_verdict compares) */
constexpr int kStreamMaxRows = 64;   /* sensors with more rows go the general way (the stream walk keeps per-row estimates in LDS) */

/* Workspace streams between the kernels of one sub-batch (see bev_exact.h for the candidate key):
 *   cand uint2 (key | height)  [nf][segs][kSeg]   candidates, one segment per (row, strip), compacted in column order;
 *                                                  segments in row-major order => concatenation = slot order
 *   ncand u32                  [nf][segs]
 *   code_main u32              [nf][emitters][bands][code_stride]   BEV codes of the slots that are NOT candidates
 *                                                  (final when the walk writes them), one list per raster band, appended
 *                                                  row by row by the strip's workgroup (no atomics)
 *   ncode u32                  [nf][emitters][bands]
 *   (k_ground_resolve appends the codes of the candidates phase C un-grounds to lists of the same kind, one set per part) */
static_assert(sizeof(bev_point_t) == 32, "bev_point_t must be 32 bytes");

struct Geometry {
    int N, H, G;       /* N_SCAN, Horizon_SCAN, GROUND_UPPER_SCAN */
    int S;             /* N * H */
    int tiles;         /* ceil(S / kTile): slot tiles of the per-slot kernels */
    int strips;        /* ceil(H / kStripCols): column strips of the walk kernel */
    int segs;          /* (G + 1) * strips: candidate segments per frame, row-major */
    int raster_bands;  /* x-bands per frame in the raster kernel (= rp.bands: coarse ones outside, fine ones in the middle) */
    int emitters;      /* strips + kResolveParts: writers of code lists per frame (the walk's strips, the resolve's parts) */
    uint32_t code_cap; /* capacity of one (emitter, band) code list: kCodeListCap, or the worst case (every slot of a strip /
                        * every candidate of a resolve part in one band) where that is smaller; a raster band with a list
                        * that does not hold its codes is computed from the ordered cloud instead */
    uint32_t code_stride; /* words from one (emitter, band) list to the next: code_cap padded to an ODD number of 256-byte pieces —
                           * lists that start a power of two apart put every writer's appends on the same few memory channels
                           * (measured: -3 % frames/s with 8-KiB strides) */
    bevx::RasterParams rp;
};

/* device-side views of one sub-batch */
struct BatchPtrs {
    const bev_point_t *pts;      /* packed input points (or ordered cloud in identity mode) */
    const FrameDesc *frames;     /* [nf] where the walk and the scan read a frame's descriptor: device memory (k_probe's copy) or the host's mapped array */
    const FrameDesc *frames_src; /* [nf] k_probe: the host's mapped array the caller's offsets were written to (16 bytes per frame over the link, once) */
    FrameDesc *frames_copy;      /* [nf] k_probe writes its copy here (== frames), or nullptr */
    FrameInfo *info;             /* [nf] (nullptr: every frame general) */
    uint32_t *est;               /* [nf][strips][N]: stream frames: estimated input position of slot (r, first column of strip - 2) */
    uint32_t *tail_list;         /* [nf][N][strips][kTailCap]: stream frames: column offset | input index << 8 of the tail points (nullptr: no stream mode) */
    uint32_t *tail_cnt;          /* [nf][strips][N] */
    int32_t *cm_par;             /* [nf][kCmParWords]: kFrameColMajorGen: the frame's direction and row bases (k_probe) */
    uint32_t *cm_sync;           /* [nf][kCmSyncWords]: kFrameColMajorGen, zeroed by k_probe: per band of two rows and strip: kCmUsedBit | the last no-return firing + 1 of either row
                                  * that the strip owns; per row: the firing + 1 whose record strip 0 put into column 0; per row: kCmUsedBit | the firing + 1 that the
                                  * strip with the wrap-around halo took for column 0 when column H - 2 fell back on it */
    uint32_t *winner;            /* [nf][S]  (win_tag << win_shift) | index+1 of the last input point per slot */
    uint32_t win_tag;            /* generation of this sub-batch in its workspace set (0: table was cleared) */
    int win_shift;               /* bits of index+1 */
    bev_point_t *ordered;        /* [nf][S] */
    uint2 *cand;                 /* [nf][segs][kSeg]: candidate key (bev_exact.h) | height */
    uint32_t *ncand;             /* [nf][segs] */
    uint32_t *code_main;         /* [nf][emitters][bands][code_stride] */
    uint32_t *ncode;             /* [nf][emitters][bands]: codes the writer had for the list (more than code_cap: the list is incomplete) */
    const uint32_t *ctx_tab;     /* [kCtxTabWords] per context: edge_x[75], edge_y[50] (BEV bins of the ground grid's cell edges), band_tab[512] bytes (x bin -> raster band) */
    float *avg;                  /* [nf][3750] */
    int8_t *gm;                  /* [nf][S] or nullptr: phase-A ground_mat */
    uint8_t *multi;              /* [nf][L*M*M] */
    uint8_t *single;             /* [nf][M*M] */
};

enum KernelId {
    K_ORDER_SCAN = 0,
    K_GATHER_GROUND,
    K_CELL_SUMS,
    K_GROUND_RESOLVE,
    K_BEV_RASTER,
    K_GATHER_ONLY,
    K_GROUND_MAT,
    K_CLOUD_CODES,
    K_ANGLE_DEBUG,
    K_FLOAT_BEV,
    K_PROJECT,
    K_TRANSFORM,
    K_PROBE,
    K_WALK_GENERAL, /* the walk through the winner table (K_GATHER_GROUND: the walk that reads in place, or the identity walk) */
    K_WALK_STRUCTURED, /* the walk over structured clouds (kFrameStructured) */
    K_WALK_COLMAJOR,   /* the walk over clouds in firing order: the plain sweep (kFrameColMajor) */
    K_WALK_COLMAJOR_GEN, /* ... any start azimuth, direction, staggered beams, no-return records (kFrameColMajorGen) */
    K_VERDICT,
    K_STAGE, /* the fused launch: a sub-batch's walk beside the later stages of the sub-batches before it (k_stage) */
    K_RF_CELLS,   /* registration front end (bev_regfront.h): cells of the top-part flatten */
    K_RF_TOP,     /* ... each cell's highest points */
    K_RF_VOXEL,   /* ... voxel grid */
    K_RF_NORMALS, /* ... 2-D normals */
    K_ICP_GRID,   /* coarse ICP (bev_icp.h): the target frames' grids */
    K_ICP,        /* ... one workgroup per (match, guess): the whole loop and the fitness */
    K_ICP_BEST,   /* ... the better guess of every match */
    K_FINE_VOXEL, /* fine stage (bev_fine.h): VoxelGrid<PointXYZIRCT> of the full clouds */
    K_FINE_GRID,  /* ... the target frames' grids */
    K_FINE_ICP,   /* ... one workgroup per match: the point-to-point loop and the fitness */
    K_KITTI_CROSSINGS, /* KITTI projection (bev_project.h): azimuths, columns, crossing lists (K_PROJECT: the MulRan / Oxford map) */
    K_KITTI_CHAIN,     /* ... the chain of accepted crossings, one wave per frame */
    K_KITTI_ASSIGN,    /* ... rings, last writer per slot */
    K_KITTI_GATHER,    /* ... the structured clouds */
    K_FLOAT_BEV_BATCH, /* the float BEV of a batch of frames under per-frame poses (bev_manip.h; K_FLOAT_BEV: one cloud) */
    K_POSED_SPLAT,     /* the 24-layer and uint8 BEVs of a batch of frames under per-frame poses (bev_posed.h): points into the workspace planes */
    K_POSED_EXPAND,    /* ... the planes into the images */
    K_SUBMAP_SPLAT,    /* the same BEVs of submaps (bev_submap.h): the points of a group's frames into their entries' grids (the images: K_POSED_EXPAND) */
    K_SUBMAP_FLOAT_SPLAT, /* the float BEV of submaps (bev_submap_float.h): the same points into their entries' grids of the output itself */
    K_SUBMAP_TARGET,   /* scan-to-map fine ICP (bev_submap_reg.h): a map's entries' moved voxel clouds and their search grid */
    K_SUBMAP_ICP,      /* ... one workgroup per match: K_FINE_ICP's loop against the map */
    K_SUBMAP_VOX_MOVE,   /* the union voxel grid of a map (bev_submap_vox.h): the entries' moved voxel clouds, concatenated */
    K_SUBMAP_VOX_KEYS,   /* ... the union's bounds and the sort keys */
    K_SUBMAP_VOX_TILE,   /* ... the sort's stages inside tiles of LDS */
    K_SUBMAP_VOX_GLOBAL, /* ... the sort's stages across tiles */
    K_SUBMAP_VOX_FINISH, /* ... voxel starts, centroids and the search grid of the thinned points */
    K_SUBMAP_VOX_OUT,    /* ... the cloud call: the maps' points and counts into the caller's arrays */
    K_SUBMAP_PN_TARGET,  /* scan-to-map coarse ICP (bev_submap_coarse.h): a map's entries' moved PointNormal rows and their search grid */
    K_SUBMAP_COARSE_ICP, /* ... one workgroup per (match, guess): K_ICP's loop against the map (the better guess: K_ICP_BEST) */
    K_SUBMAP_PN_MOVE,    /* the union voxel grid and 2-D normals of a PointNormal map (bev_submap_pn_vox.h): the entries' moved rows, concatenated */
    K_SUBMAP_PN_KEYS,    /* ... the union's bounds and the sort keys (the sort: K_SUBMAP_VOX_TILE, K_SUBMAP_VOX_GLOBAL) */
    K_SUBMAP_PN_FINISH,  /* ... voxel starts, voxel indices and centroids */
    K_SUBMAP_PN_NORMALS, /* ... the normals of the thinned points over a 3-D window of the union's grid */
    K_SUBMAP_PN_GRID,    /* ... the search grid of the thinned rows */
    K_SUBMAP_PN_OUT,     /* ... the cloud call: the maps' rows and counts into the caller's arrays */
    K_SUBMAP_TOP_KEYS,     /* the top part over the union of a map's moved full clouds (bev_submap_top.h): the moved records' keys, the cells' counts */
    K_SUBMAP_TOP_CELLS,    /* ... the cells' ranks and the selection's size */
    K_SUBMAP_TOP_HIST,     /* ... the radix select: one digit's histogram per cell */
    K_SUBMAP_TOP_SCAN,     /* ... the radix select: the cells' buckets, prefixes and thresholds */
    K_SUBMAP_TOP_COMPACT,  /* ... the selected keys (the sort: K_SUBMAP_VOX_TILE, K_SUBMAP_VOX_GLOBAL) */
    K_SUBMAP_TOP_ROWS,     /* ... the rows of top(g) from the sorted keys */
    K_SUBMAP_TOP_OVERFLOW, /* ... the voxel grid's overflow branch: top(g) kept for the normals' full scan */
    K_SUBMAP_GRID_BOUNDS,  /* a map's search grid sized to the map (bev_submap_grid.h): the parts' bounds */
    K_SUBMAP_GRID_HEADER,  /* ... the grid's header */
    K_SUBMAP_GRID_COUNT,   /* ... the cells' counts in global memory */
    K_SUBMAP_GRID_SUMS,    /* ... the scan: the tiles' sums */
    K_SUBMAP_GRID_SCAN,    /* ... the scan: the cells' offsets and cursors */
    K_SUBMAP_GRID_SCATTER, /* ... the searchable points by cell */
    K_SUBMAP_ICP_WIDE,        /* K_SUBMAP_ICP against such a grid */
    K_SUBMAP_COARSE_ICP_WIDE, /* K_SUBMAP_COARSE_ICP against such a grid, its offsets in global memory */
    K_PAIRGRID_DESC, /* the pair calls' search grids sized to the cloud (bev_pair_grid.h): the targets' point counts */
    K_FINE_ICP_WIDE, /* K_FINE_ICP against such a grid */
    K_ICP_WIDE,      /* K_ICP against such a grid, its offsets in global memory */
    K_PLACE_SPLAT,   /* place retrieval (bev_place.h): the points of frames, or of maps' entries, into polar max-height planes */
    K_PLACE_FINISH,  /* ... the planes into descriptor bytes, unit columns and column masks */
    K_PLACE_PAIRS,   /* ... the best shift of every (query, candidate) pair */
    K_PLACE_TOPK,    /* ... the best top_k candidates of every query */
    K_VERIFY_MOVE,   /* verification of registered matches (bev_verify.h): the moved query of every match and its search grid */
    K_VERIFY_COUNT,  /* ... the inlier counts of both directions */
    K_ALIGN_GRID,    /* translation guess of retrieved pairs (bev_align.h): the candidates' height grids, maxima per cell */
    K_ALIGN_FINISH,  /* ... their bytes and sums of squares */
    K_ALIGN_HIT,     /* ... every shift of one (hit, flip, k) hypothesis and the best of them */
    K_ALIGN_PICK,    /* ... per hit: the order over k, the sub-cell offsets, the results, the detail and best */
    K_COUNT
};
const char *kernel_name(int id);
/* smallest of 8, 16, 32, 64 uniform bands whose LDS planes (2 * (M / bands) * M * 4 B + the list prefix) fit; 0 if none does */
int raster_bands_for(int mat_size);

/* One fused launch (k_stage): the column walk of one sub-batch and, as further workgroups of the same grid, phase B of the
 * sub-batch before it, phase C of the one before that and the rasters of the one before that — every dependency between
 * stages of one sub-batch is the order of launches on one stream; nothing inside a launch waits for anything.  nf == 0: the
 * stage is absent from this launch. */
struct StagePart {
    BatchPtrs b;
    int nf;
};
struct StageArgs {
    Geometry g;
    StagePart walk, sums, resolve, raster;
    uint32_t want_mode;           /* of the walk part (see launch_gather_ground) */
    int want_multi, want_single;  /* of the raster part */
    int lead;                     /* group slots (8 frames each) by which the walk's workgroups precede the other stages' in the grid */
};
/* source: the walk part's (see launch_gather_ground; ignored when a.walk.nf == 0) */
void launch_stage(const StageArgs &a, int source, hipStream_t st);
size_t stage_lds_bytes(const Geometry &g, int source);

/* launchers (bev_kernels.hip) — all asynchronous on `st` */
/* the frames that are not read in place: general ones and (after k_verdict) those whose verification failed */
void launch_order_scan(const Geometry &g, const BatchPtrs &b, int nf, uint32_t max_pts, bool thin, hipStream_t st);
/* the column walk and where it takes its points from.  source
 *   kSrcGather       through the winner table of the order scan (the frames that are not read in place: pass kFrameGeneral);
 *   kSrcIdentity     b.pts already is the ordered cloud (bev_mark_ground);
 *   kSrcInPlace      a sorted prefix read in place (frames of mode kFrameStream: pass mode = kFrameStream);
 *   kSrcStructured   structured clouds (kFrameStructured);
 *   kSrcColMajor     the plain sweep in firing order (kFrameColMajor);
 *   kSrcColMajorGen  firing order in its general form (kFrameColMajorGen)
 * — the last four take the frames of the mode passed */
enum : int { kSrcGather = 0, kSrcIdentity = 1, kSrcInPlace = 2, kSrcStructured = 3, kSrcColMajor = 4, kSrcColMajorGen = 5 };
void launch_gather_ground(const Geometry &g, const BatchPtrs &b, int nf, int source, uint32_t mode, hipStream_t st);
void launch_probe(const Geometry &g, const BatchPtrs &b, int nf, bool allow_stream, int layout_hint /* 0, kFrameStructured or kFrameColMajor */, hipStream_t st);
void launch_verdict(const Geometry &g, const BatchPtrs &b, int nf, uint32_t *host_hint, hipStream_t st);
void launch_gather_only(const Geometry &g, const BatchPtrs &b, int nf, hipStream_t st);
void launch_cell_sums(const Geometry &g, const BatchPtrs &b, int nf, hipStream_t st);
void launch_ground_resolve(const Geometry &g, const BatchPtrs &b, int nf, hipStream_t st);
/* the rasters of a sub-batch from its code lists */
void launch_bev_raster(const Geometry &g, const BatchPtrs &b, bool want_multi, bool want_single, int nf, hipStream_t st);
/* rasters of ONE arbitrary cloud from a dense code array (bev_multi_bev / bev_single_bev) */
void launch_bev_raster_dense(const Geometry &g, const uint32_t *codes, uint32_t n_codes, uint8_t *multi, uint8_t *single,
                             hipStream_t st);
void launch_ground_mat(const Geometry &g, const BatchPtrs &b, int8_t *out, int nf, hipStream_t st);
void launch_cloud_codes(const Geometry &g, const bev_point_t *cloud, uint32_t n, uint32_t *codes, hipStream_t st);
void launch_float_bev(const bev_point_t *cloud, uint32_t n, float interval, int M, bool skip_label0, float *grid,
                      hipStream_t st);
void launch_transform(const bev_point_t *cloud, uint32_t n, const float m[12], bev_point_t *out, hipStream_t st);
/* ---- range-image projection of raw returns (bev_project.h) ---- */
/* one frame of a projection call (device table of n_frames + 1 entries; the last one carries the total block count) */
struct ProjFrame {
    uint64_t off;  /* first return of the frame in the packed input (16 bytes per return) — and, kinds 0 / 1, its first record in the output */
    uint32_t n;    /* returns */
    uint32_t blk0; /* map kernels: workgroups before this frame's first (kProjBlock returns per workgroup) */
};
constexpr int kProjPerThread = 4;
constexpr int kProjBlock = 256 * kProjPerThread; /* returns per workgroup of the map kernel */
/* MulRan / Oxford: one launch for all frames; `blocks` = tab[nf].blk0 */
void launch_project_batch(int kind, const float *xyzi, const ProjFrame *tab, int nf, uint32_t blocks, bev_point_t *out,
                          hipStream_t st);
/* KITTI projection workspace (device) of one launch group, per frame: header with the chain of accepted crossings,
 * per-point column, per-block crossing lists, winner table of the 64 x 2083 structured cloud */
constexpr int kKittiGroup = BEV_PROJECT_KITTI_GROUP; /* frames per launch group */
struct KittiHeader {
    int32_t ring0;
    uint32_t n_links;
    uint32_t link[68];
};
struct KittiWork {
    KittiHeader *hdr; /* [group] */
    int32_t *col;     /* [group][n_cap] */
    uint32_t *cnt;    /* [group][blocks_cap], blocks_cap = ceil(n_cap / 256) */
    uint32_t *pos;    /* [group][blocks_cap][128] */
    uint32_t *winner; /* [group][64 * 2083] */
    uint32_t n_cap, blocks_cap;
};
/* the four steps for the nf <= group frames of tab (n_max: the longest of them); frame g's structured cloud at
 * out + g * 64 * 2083; w.winner[0 .. nf * 64 * 2083) zeroed by the caller on the same stream.  step 0 .. 3: crossings, chain,
 * assign, gather (a launch each, so that each has its own profile row: K_KITTI_CROSSINGS + step) */
void launch_project_kitti(int step, const float *xyzi, const ProjFrame *tab, int nf, uint32_t n_max, const KittiWork &w,
                          bev_point_t *out, hipStream_t st);
/* ---- float max-height BEV of a batch of frames (bev_manip.h) ----
 * one launch for all frames and poses: tab as for launch_project_batch (offsets and counts in records), poses nf * n_poses
 * row-major 3 x 4 matrices (n_poses == 0: none, raw coordinates), grids nf * max(1, n_poses) * M * M floats, zeroed by the
 * caller on the same stream */
void launch_float_bev_batch(const bev_point_t *clouds, const ProjFrame *tab, int nf, uint32_t blocks, const float *poses,
                            int n_poses, float interval, int M, bool skip_label0, float *grids, hipStream_t st);
/* ---- 24-layer and uint8 BEVs of a batch of frames under per-frame poses (bev_posed.h) ----
 * one launch group: the nf frames from tab[0] on (tab: a piece of the call's table, as for launch_project_batch; blocks: the
 * workgroups of these frames, tab[nf].blk0 - tab[0].blk0), poses nf * n_poses matrices (n_poses == 0: none), planes
 * nf * max(1, n_poses) grids of 2 * M * M words, zeroed by the caller on the same stream; then the planes of n_grids grids into
 * images n_grids of multi / single (nullptr: not wanted) */
void launch_posed_splat(const bev_point_t *clouds, const ProjFrame *tab, int nf, uint32_t blocks, const float *poses, int n_poses,
                        const Geometry &g, uint32_t *planes, hipStream_t st);
void launch_posed_expand(const Geometry &g, const uint32_t *planes, int n_grids, uint8_t *multi, uint8_t *single, hipStream_t st);
/* ---- the same BEVs of submaps: windows of posed frames rastered into one grid per map (bev_submap.h) ----
 * a piece of one launch group of the plan (bev_submap_plan.h): the nf rows from rows[0] on (bevsub::Frame, read as ProjFrame)
 * with their entry starts ent0 (nf + 1 values), blocks = rows[nf].blk0 - rows[0].blk0 workgroups; entries: the group's
 * (bevsub::Entry); planes: the group's grids, zeroed by the caller on the same stream.  The images: launch_posed_expand. */
void launch_submap_splat(const bev_point_t *clouds, const void *rows, const uint32_t *ent0, int nf, uint32_t blocks,
                         const void *entries, const Geometry &g, uint32_t *planes, hipStream_t st);
/* ---- the float max-height BEV of submaps (bev_submap_float.h) ----
 * rows, ent0, blocks and entries as for launch_submap_splat, of the call's ONE launch group; grids: one grid of M * M floats
 * per map, the atomics' target, zeroed by the caller on the same stream */
void launch_submap_float_splat(const bev_point_t *clouds, const void *rows, const uint32_t *ent0, int nf, uint32_t blocks,
                               const void *entries, float interval, int M, bool skip_label0, float *grids, hipStream_t st);
/* ---- place retrieval: polar descriptors and the search over pairs and rotations (bev_place.h) ---- */
struct PlaceShape { /* a descriptor's shape and what a point's value needs (the ring edges go up beside the frame table) */
    int n_rings, n_sectors, skip_label0;
    float lidar_to_ground;
};
constexpr int kPlaceWords = 8; /* words of a unit column: 32 rings, four to a word */
constexpr int kPlaceTile = 64; /* candidates per workgroup of k_place_pairs */
/* the opaque per-descriptor record of the C ABI (bev_place_desc_handle_bytes): unit[s] column s's unit values, ring r in byte
 * r % 4 of word r / 4, zero past n_rings and in the columns past n_sectors; mask: bit s set where column s is not empty */
struct alignas(64) PlaceHandle {
    uint32_t unit[64][kPlaceWords];
    uint64_t mask;
    uint32_t pad[14];
};
static_assert(sizeof(PlaceHandle) == 2112, "the device reads this layout");
/* rows, ent0, blocks and entries as for launch_submap_float_splat (ent0 == nullptr: no maps, row f's raw points into plane f);
 * edge2: n_rings + 1 floats on the device; planes: n_rings * n_sectors words per descriptor, zeroed by the caller on the stream */
void launch_place_splat(const bev_point_t *clouds, const void *rows, const uint32_t *ent0, int nf, uint32_t blocks,
                        const void *entries, const float *edge2, const PlaceShape &ps, uint32_t *planes, hipStream_t st);
/* n_desc planes into desc (nullptr: not wanted) and units (nullptr: not wanted) */
void launch_place_finish(const uint32_t *planes, int n_desc, const PlaceShape &ps, uint8_t *desc, PlaceHandle *units, hipStream_t st);
/* queries [q0, q0 + nq) of uq against candidates 0 .. limit[q] - 1 of udb (limit == nullptr: n_db; a device array indexed by
 * q): pairs[(q - q0) * n_db + c] = the pair's best (S, cnt | shift << 16); then their top_k hits into hits + q * top_k */
void launch_place_pairs(const PlaceHandle *uq, int q0, int nq, const PlaceHandle *udb, int n_db, const int32_t *limit,
                        const PlaceShape &ps, uint2 *pairs, hipStream_t st);
void launch_place_topk(const uint2 *pairs, int q0, int nq, int n_db, const int32_t *limit, const PlaceShape &ps, int top_k,
                       bev_place_hit_t *hits, hipStream_t st);
void launch_angle_debug(const float *dx, const float *dy, const float *dz, uint8_t *out, size_t n, hipStream_t st);
/* element i of function `id` (bev_exact_eval.h) for i < n: in its device arrays, prm its 12 floats (nullptr: zeros), out n * out_words words */
void launch_exact_eval(int id, const void *const in[4], const float *prm, uint32_t *out, uint32_t out_words, size_t n, hipStream_t st);
/* ---- registration front end (bev_regfront.h; DESIGN.md "Registration front end") ---- */
constexpr int kRfThreads = 256;
constexpr int kRfGrid = 10;                  /* NUM_GRID_X / NUM_GRID_Y of extractTopAndFlatten (TopPartRegistration.cpp:83-84) */
constexpr int kRfCells = kRfGrid * kRfGrid;
constexpr int kRfMinCellPoints = 20;         /* MIN_GRID_POINTS_SIZE (:90) */
constexpr int kRfLdsKeys = 8192;             /* keys a workgroup sorts in LDS (64 KiB); more: in its global scratch region */
struct RfFrameMeta {
    uint32_t m;        /* top-part points of the frame (the voxel stage's input count) */
    uint32_t nv;       /* voxels (the normal stage's point count) */
    uint32_t windowed; /* the voxels are sorted by index i + j * div_x: neighbours lie in a contiguous window of rows */
    uint32_t div_x, div_y;
    uint32_t _pad[3];
};
/* per frame: P = max(max_points, S) input points, Q = P points between the stages */
struct RfWork {
    uint64_t *keys;      /* [nf][P]        top-part sort keys, bucketed by cell */
    uint64_t *scr;       /* [nf][2P]       global sort scratch (cells / voxel sorts too large for LDS) */
    uint32_t *cell_cnt;  /* [nf][100] */
    uint32_t *cell_off;  /* [nf][101]      bucket offsets */
    uint32_t *out_off;   /* [nf][101]      output offsets of the cells' top points */
    float4 *flat;        /* [nf][Q]        flattened top points (PointXYZ, pad 0) */
    float4 *vpts;        /* [nf][Q]        voxel centroids */
    uint32_t *vidx;      /* [nf][Q]        voxel index of each centroid */
    uint32_t *vstart;    /* [nf][Q + 1]    first sorted key of each voxel */
    RfFrameMeta *meta;   /* [nf] */
    size_t P, Q;
};
struct RfIn {
    const bev_point_t *pts;
    const uint64_t *offs; /* [nf + 1] element offsets (device), or nullptr: frame f = pts + f * stride, n_uniform points */
    size_t stride;
    uint32_t n_uniform;
};
/* phase 0: k_rf_cells, 1: k_rf_top */
void launch_rf_top(const RfIn &in, const RfWork &w, int nf, hipStream_t st, int phase);
void launch_rf_voxel(const RfWork &w, int nf, float leaf, uint32_t *counts, hipStream_t st);
void launch_rf_normals(const RfWork &w, int nf, uint32_t max_points, float radius, float leaf, const float vp[2],
                       bool point_normal, float *out, size_t out_stride, hipStream_t st);

/* ---- coarse point-to-plane ICP (bev_icp.h) ---- */
constexpr int kIcpThreads = 256;
constexpr int kIcpGridMax = 64;                       /* cells per axis of a target frame's grid */
constexpr int kIcpCells = kIcpGridMax * kIcpGridMax;
constexpr int kIcpChunkSlots = 32;                    /* 64-point chunk sums a workgroup holds in LDS at once */
constexpr int kIcpProblemsPerLaunch = 1024;           /* problems of one k_icp launch (= transformed clouds in scratch) */
struct IcpGridHdr {
    float minx, miny, inv_s, s; /* cell (floor((x - minx) * inv_s), ...) clamped; square cells of side s */
    int32_t nx, ny;
    float mag;                  /* largest |coordinate| of the bounds (the ring bound's rounding margin) */
    uint32_t n;                 /* searchable points */
};
struct IcpProblem {
    uint32_t src_frame, tgt_frame, tgt_slot, result;
    float guess[16]; /* row-major */
};
/* per target slot: header, nx * ny + 1 cell offsets, the searchable points (x, y, z, index bits) by cell; per problem of
 * a launch: the transformed source */
struct IcpWork {
    IcpGridHdr *hdr;    /* [slots] */
    uint32_t *cell_off; /* [slots][kIcpCells + 1] */
    float4 *sorted;     /* [slots][stride] */
    float4 *cur;        /* [kIcpProblemsPerLaunch][stride] */
};
void launch_icp_grid(const float *pn, size_t stride, const uint32_t *counts, const uint32_t *slot_frame, int n_slots,
                     const IcpWork &w, hipStream_t st);
void launch_icp(const float *pn, size_t stride, const uint32_t *counts, const IcpProblem *probs, int n,
                const IcpWork &w, const bev_icp_params_t &prm, bev_icp_result_t *results, hipStream_t st);
void launch_icp_best(const bev_icp_result_t *res, int n_matches, int32_t *best, hipStream_t st);

/* ---- fine stage: VoxelGrid<PointXYZIRCT> and point-to-point ICP (bev_fine.h) ---- */
constexpr int kFineThreads = 256;
constexpr int kFineGridMax = 128;                     /* cells per axis of a target frame's grid (counts: 64 KiB of LDS) */
constexpr int kFineCells = kFineGridMax * kFineGridMax;
constexpr int kFineSvdSweeps = 64;                    /* Jacobi sweeps of the 3 x 3 SVD at most (never reached on finite input) */
constexpr int kFineProblemsPerLaunch = 1024;          /* problems of one k_fine_icp launch (= transformed clouds in scratch) */
constexpr int kFineVoxelGroup = 256;                  /* frames of one k_fine_voxel launch (= sort scratch regions) */
/* a frame of the call: its records are pts + off, n of them (n <= Pn) */
struct FineSlot {
    uint64_t off;
    uint32_t n, _pad;
};
/* src / tgt: slots; coarse_match != ~0: the guess is coarse[2 m + best[m]].T, else guess */
struct FineProblem {
    uint32_t src_slot, tgt_slot, result, coarse_match;
    float guess[16]; /* row-major */
};
/* per slot: the voxel grid's records and count, the grid (header, offsets, the searchable points by cell); per frame of a
 * voxel launch: the sort keys and voxel starts; per problem of an ICP launch: the transformed source, its correspondences */
struct FineWork {
    bev_point_t *vox;   /* [slots][Pn] */
    uint32_t *vox_n;    /* [slots] */
    uint64_t *keys;     /* [kFineVoxelGroup][Kn] */
    uint32_t *vstart;   /* [kFineVoxelGroup][Pn + 1] */
    IcpGridHdr *hdr;    /* [slots] */
    uint32_t *cell_off; /* [slots][kFineCells + 1] */
    float4 *sorted;     /* [slots][Pn] */
    float4 *cur;        /* [kFineProblemsPerLaunch][Pn] */
    uint32_t *corr;     /* [kFineProblemsPerLaunch][Pn] */
    size_t Pn, Kn;      /* Kn: the smallest power of two >= Pn */
};
/* slots slot0 ... slot0 + n - 1 (n <= kFineVoxelGroup) */
void launch_fine_voxel(const bev_point_t *pts, const FineSlot *slots, int slot0, int n, const FineWork &w, float leaf,
                       hipStream_t st);
void launch_fine_grid(int n_slots, const FineWork &w, hipStream_t st);
void launch_fine_icp(const FineProblem *probs, int n, const FineWork &w, const bev_icp_result_t *coarse,
                     const int32_t *best, const bev_icp_params_t &prm, bev_icp_result_t *results, hipStream_t st);

/* ---- scan-to-map fine ICP (bev_submap_reg.h, bev_submap_reg_plan.h) ----
 * the maps of ONE launch group of the plan: a map's points at its pt0, its header and cell offsets at its index in the group */
struct SubmapRegWork {
    float4 *pts;        /* [the group's points]   the entries' moved voxel points: x, y, z */
    float4 *sorted;     /* [the group's points]   the searchable ones by cell (x, y, z, index bits) */
    IcpGridHdr *hdr;    /* [the group's maps] */
    uint32_t *cell_off; /* [the group's maps][kFineCells + 1] */
};
/* maps / entries: the plan's tables (bevsubreg::Map, ::Entry); the n_maps maps from map0 on; ent_start: a word per entry of
 * the call; w: the voxel clouds (vox, vox_n, Pn) */
void launch_submap_target(const void *maps, uint32_t map0, int n_maps, const void *entries, const FineWork &w,
                          uint32_t *ent_start, const SubmapRegWork &t, hipStream_t st);
/* n <= kFineProblemsPerLaunch problems whose tgt_slot is a map's index in the plan (all in the group from map0 on) */
void launch_submap_icp(const FineProblem *probs, int n, const void *maps, uint32_t map0, const FineWork &w,
                       const SubmapRegWork &t, const bev_icp_result_t *coarse, const int32_t *best, const bev_icp_params_t &prm,
                       bev_icp_result_t *results, hipStream_t st);

/* ---- the union voxel grid of a map (bev_submap_vox.h, bev_submap_vox_plan.h) ----
 * the maps of ONE launch group of a plan with union_voxel */
struct SubvoxHdr {
    uint32_t n;        /* points of the concatenation */
    uint32_t np2;      /* keys to sort: the smallest power of two >= n, or 0: nothing to sort */
    uint32_t nf;       /* finite points among them */
    uint32_t overflow; /* the union's grid has more than INT32_MAX voxels: the target is the concatenation */
    uint32_t n_out;    /* points of the target */
    uint32_t div[3];   /* bev_submap_pn_vox.h: the union grid's divisions along x, y, z where the keys are sorted; else 0 */
};
struct SubmapVoxWork {
    float4 *moved;        /* [the group's points]        the concatenation: a map's at its pt0 */
    uint64_t *keys;       /* [the group's keys]          a map's at key0[its index in the plan] */
    uint32_t *vstart;     /* [the group's points + maps] a map's capacity + 1 words at pt0 + its index in the group */
    SubvoxHdr *vh;        /* [the group's maps] */
    const uint64_t *key0; /* [the plan's maps]           device table */
};
void launch_submap_vox_move(const void *maps, uint32_t map0, int n_maps, const void *entries, const FineWork &w,
                            uint32_t *ent_start, const SubmapVoxWork &v, hipStream_t st);
void launch_submap_vox_keys(const void *maps, uint32_t map0, int n_maps, const SubmapVoxWork &v, float map_leaf, hipStream_t st);
/* one launch of bevsubvox::schedule: tiles workgroups along x for each of the n_maps maps */
void launch_submap_vox_stage(uint32_t kind, uint32_t k, uint32_t j, uint32_t map0, int n_maps, uint32_t tiles,
                             const SubmapVoxWork &v, hipStream_t st);
/* t.pts: the thinned points; t.hdr == nullptr: no search grid (the cloud call) */
void launch_submap_vox_finish(const void *maps, uint32_t map0, int n_maps, const SubmapVoxWork &v, const SubmapRegWork &t,
                              hipStream_t st);
/* the cloud calls of this section and of §6q.  src: the group's array that holds the targets (moved or thinned), rows of
 * row_f4 float4 (points: 1, PointNormal rows: 3); out, counts: the caller's, indexed by map of the plan, stride in rows */
void launch_submap_out(const void *maps, uint32_t map0, int n_maps, uint32_t parts, const SubvoxHdr *vh, const void *src,
                       void *out, uint64_t stride, uint32_t *counts, uint32_t row_f4, hipStream_t st);

/* ---- scan-to-map coarse ICP (bev_submap_coarse.h, bev_submap_reg_plan.h) ----
 * the maps of ONE launch group of the plan: a map's rows at its pt0, its header and cell offsets at its index in the group */
struct SubmapCoarseWork {
    float *rows;        /* [the group's rows][12]  the entries' moved PointNormal rows */
    float4 *sorted;     /* [the group's rows]      the searchable ones by cell (x, y, z, index bits) */
    IcpGridHdr *hdr;    /* [the group's maps] */
    uint32_t *cell_off; /* [the group's maps][kIcpCells + 1] */
    float4 *cur;        /* [kIcpProblemsPerLaunch][stride] */
};
/* maps / entries: the plan's tables, an entry's slot word holding its FRAME; the n_maps maps from map0 on; pn, stride, counts:
 * the call's frames; ent_start: a word per entry of the call */
void launch_submap_pn_target(const void *maps, uint32_t map0, int n_maps, const void *entries, const float *pn, size_t stride,
                             const uint32_t *counts, uint32_t *ent_start, const SubmapCoarseWork &t, hipStream_t st);
/* n <= kIcpProblemsPerLaunch problems whose tgt_slot is a map's index in the plan (all in the group from map0 on) */
void launch_submap_coarse_icp(const float *pn, size_t stride, const uint32_t *counts, const IcpProblem *probs, int n,
                              const void *maps, uint32_t map0, const SubmapCoarseWork &t, const bev_icp_params_t &prm,
                              bev_icp_result_t *results, hipStream_t st);

/* ---- the union voxel grid and 2-D normals of a PointNormal map (bev_submap_pn_vox.h) ----
 * the maps of ONE launch group of a plan with point_normal and union_voxel; the target rows are SubmapCoarseWork::rows */
struct SubmapPnVoxWork {
    float *moved;    /* [the group's rows][12]  the concatenation: a map's at its pt0 */
    SubmapVoxWork v; /* keys, vstart, vh, key0 as in §6l (the sort's kernels read them); v.moved is not used */
    uint32_t *vidx;  /* [the group's rows]      a thinned point's voxel index in the union's grid */
    float4 *vpos;    /* [the group's rows]      a thinned point's position */
};
void launch_submap_pn_move(const void *maps, uint32_t map0, int n_maps, const void *entries, const float *pn, size_t stride,
                           const uint32_t *counts, uint32_t *ent_start, const SubmapPnVoxWork &p, hipStream_t st);
void launch_submap_pn_keys(const void *maps, uint32_t map0, int n_maps, const SubmapPnVoxWork &p, float pn_leaf, hipStream_t st);
/* target: the group's target rows (thinned positions go to p.vpos; the overflow branch copies the moved rows to target) */
void launch_submap_pn_finish(const void *maps, uint32_t map0, int n_maps, const SubmapPnVoxWork &p, float *target, hipStream_t st);
/* parts: workgroups of 256 thinned points along x for each of the n_maps maps (the largest capacity's) */
void launch_submap_pn_normals(const void *maps, uint32_t map0, int n_maps, uint32_t parts, const SubmapPnVoxWork &p, float radius,
                              float pn_leaf, const float vp[2], float *target, hipStream_t st);
void launch_submap_pn_grid(const void *maps, uint32_t map0, int n_maps, const SubvoxHdr *vh, const SubmapCoarseWork &t,
                           hipStream_t st);

/* ---- the top part over the union of a map's moved full clouds (bev_submap_top.h) ----
 * the maps of ONE launch group of a plan with top_union (and point_normal, union_voxel): a map's rows (SubmapPnVoxWork::moved and
 * everything behind it) are counted in rows of top(g), its keys in records of the union */
constexpr uint32_t kTopIndexBits = 25;               /* a record's index in the union: BEV_SUBMAP_TOP_MAX_UNION = 2^24 records */
constexpr uint32_t kTopKeyBits = 32 + kTopIndexBits; /* rf_z_desc_key << 25 | index; the cell above them */
constexpr uint32_t kTopDigitBits = 6, kTopDigits = 1u << kTopDigitBits; /* of the radix select: 10 digits, the first of 3 bits */
constexpr uint32_t kTopHistWords = kRfCells * kTopDigits;               /* 25 KiB of LDS: six workgroups per CU */
struct SubtopCells {
    uint32_t cnt[kRfCells];    /* kept records of the cell (zeroed by the caller on the same stream) */
    uint32_t k[kRfCells];      /* round(0.2f * cnt) where cnt >= 20, else 0 */
    uint32_t rank[kRfCells];   /* the rank sought among the keys that share the prefix; 0: the cell is finished, or not kept */
    uint64_t prefix[kRfCells]; /* the digits found so far */
    uint64_t thr[kRfCells];    /* finished: the cell's keys (57 bits) at or below it are its selection */
    uint32_t n_sel;            /* sum of k: rows of top(g) */
    uint32_t cursor;           /* slots handed out (zeroed by the caller) */
    uint32_t open;             /* cells not finished */
    uint32_t _pad;
};
struct SubmapTopWork {
    uint64_t *ukeys;    /* [the group's union records] a map's at u0[its index in the plan] */
    SubtopCells *cells; /* [the group's maps] */
    uint32_t *hist;     /* [the group's maps][kTopHistWords]  zeroed by the caller on the same stream, zero again after every digit */
    const uint64_t *u0; /* [the plan's maps]  device table */
};
/* maps / entries / slots: the plan's tables (an entry's pad words: its first union index, its records); parts: workgroups
 * along x for each of the n_maps maps from map0 on */
void launch_submap_top_keys(const void *maps, uint32_t map0, int n_maps, uint32_t parts, const void *entries, const void *slots,
                            const bev_point_t *clouds, const SubmapTopWork &t, hipStream_t st);
void launch_submap_top_cells(int n_maps, const SubmapTopWork &t, SubvoxHdr *vh, hipStream_t st);
/* one digit of the select at `shift`: its histogram (scan false), then its scan (true) */
void launch_submap_top_digit(const void *maps, uint32_t map0, int n_maps, uint32_t parts, const void *entries,
                             const SubmapTopWork &t, uint32_t shift, bool scan, hipStream_t st);
void launch_submap_top_compact(const void *maps, uint32_t map0, int n_maps, uint32_t parts, const void *entries,
                               const SubmapTopWork &t, const SubmapVoxWork &v, hipStream_t st);
void launch_submap_top_rows(const void *maps, uint32_t map0, int n_maps, uint32_t parts, const void *entries, const void *slots,
                            const bev_point_t *clouds, const SubmapTopWork &t, const SubmapPnVoxWork &p, hipStream_t st);
void launch_submap_top_overflow(const void *maps, uint32_t map0, int n_maps, const SubmapPnVoxWork &p, hipStream_t st);

/* ---- a map's search grid sized to the map (bev_submap_grid.h) ----
 * the maps of ONE launch group of a plan with grid_cap > 0: a map's offsets and counters at cell0[its index in the plan];
 * the pair calls' targets (§6t) in the same terms */
constexpr uint32_t kSubgridParts = 256;     /* workgroups over a map's points at most (bevsubreg::kGridParts) */
constexpr uint32_t kSubgridScanParts = 256; /* tiles of 4096 cells of a map at most (bevsubreg::kGridScanParts) */
struct SubmapGridWork {
    IcpGridHdr *hdr;        /* [the group's maps] */
    uint32_t *off;          /* [the group's cells]  nx * ny + 1 offsets per map */
    uint32_t *cnt;          /* [the group's cells]  the counters, then the cursors; zeroed by the caller on the same stream */
    float4 *sorted;         /* [the group's points] the searchable points by cell: a map's at its pt0 */
    float4 *part_bounds;    /* [the group's maps][kSubgridParts]      min x, min y, max x, max y */
    uint32_t *part_sum;     /* [the group's maps][kSubgridScanParts] */
    const uint64_t *cell0;  /* [the plan's maps]    device table */
};
/* where the build reads its targets' points, a target's at its pt0: exactly one of the three is set, {pts, recs, rows} */
struct SubgridSource {
    const float4 *pts;       /* float4 points (scan-to-map, fine) */
    const bev_point_t *recs; /* 32-byte records (pair, fine: the slots' voxel clouds) */
    const float *rows;       /* PointNormal rows (both coarse stages) */
};
/* one step of the build for the n_maps maps from map0 on: 0 bounds, 1 header, 2 count, 3 sums, 4 scan, 5 scatter.  parts:
 * workgroups over the largest map's points; tiles: over the largest map's cells; cap: the cap of cells per axis; vh: the maps'
 * point counts (n_out) */
void launch_subgrid(int step, const void *maps, uint32_t map0, int n_maps, uint32_t parts, uint32_t tiles, int cap,
                    const SubvoxHdr *vh, const SubgridSource &src, const SubmapGridWork &w, hipStream_t st);

/* ---- the pair calls' search grids sized to the cloud (bev_pair_grid.h, bev_pair_grid_plan.h) ----
 * maps: the host's table of the call's targets (bevsubreg::Map: pt0 the target's first point, ent0 its slot or frame); the build
 * is §6s's over the n targets from t0 on, w's hdr and off pointing at target t0's, w.cell0 at the table of first counters */
/* the targets' point counts into vh: vox_n[t] (fine), or min(counts[ent0], stride) */
void launch_pairgrid_desc(const void *maps, int n, const uint32_t *vox_n, const uint32_t *counts, size_t stride, SubvoxHdr *vh,
                          hipStream_t st);

/* ---- the ICP loops against a grid of either build (bev_wide_icp.h) ---- */
/* launch_submap_icp and launch_submap_coarse_icp with t.cell_off the group's offsets and cell0 the plan's table of bases */
void launch_submap_icp_wide(const FineProblem *probs, int n, const void *maps, uint32_t map0, const FineWork &w,
                            const SubmapRegWork &t, const uint64_t *cell0, const bev_icp_result_t *coarse, const int32_t *best,
                            const bev_icp_params_t &prm, bev_icp_result_t *results, hipStream_t st);
void launch_submap_coarse_icp_wide(const float *pn, size_t stride, const uint32_t *counts, const IcpProblem *probs, int n,
                                   const void *maps, uint32_t map0, const SubmapCoarseWork &t, const uint64_t *cell0,
                                   const bev_icp_params_t &prm, bev_icp_result_t *results, hipStream_t st);
/* launch_fine_icp and launch_icp with w.cell_off the wide table: a slot's offsets at slot * off_words; launch_icp_wide reads
 * w.sorted by FRAME */
void launch_fine_icp_wide(const FineProblem *probs, int n, const FineWork &w, uint64_t off_words, const bev_icp_result_t *coarse,
                          const int32_t *best, const bev_icp_params_t &prm, bev_icp_result_t *results, hipStream_t st);
void launch_icp_wide(const float *pn, size_t stride, const uint32_t *counts, const IcpProblem *probs, int n, const IcpWork &w,
                     uint64_t off_words, const bev_icp_params_t &prm, bev_icp_result_t *results, hipStream_t st);

/* ---- verification of registered matches: two-way inlier counts (bev_verify.h) ---- */
constexpr int kVerifyProblemsPerLaunch = 1024; /* matches of one launch group (= moved queries and their grids in scratch) */
constexpr uint32_t kVerifySlice = 256;         /* points of one k_verify_count workgroup (BEV_VERIFY_SLICE; no result depends on it) */
/* a match of a launch group: its query's slot, its target's grid (the index of its header and of its kFineCells + 1 offsets) and
 * first searchable point behind VerifyTarget's arrays, its record in the call's d_results and d_verify */
struct VerifyProblem {
    uint32_t src_slot, tgt_grid, result, _pad;
    uint64_t tgt_pt0;
};
/* the targets' grids as their builders left them: k_fine_grid's per slot (pair), k_submap_target's or k_submap_vox_finish's per
 * map of a launch group (scan-to-map) */
struct VerifyTarget {
    const IcpGridHdr *hdr;
    const uint32_t *cell_off;
    const float4 *sorted;
};
/* per match of a launch group: the moved query, its searchable points by cell, its grid's offsets and header */
struct VerifyWork {
    float4 *moved;     /* [kVerifyProblemsPerLaunch][Pn] */
    float4 *qsorted;   /* [kVerifyProblemsPerLaunch][Pn] */
    uint32_t *qoff;    /* [kVerifyProblemsPerLaunch][kFineCells + 1] */
    IcpGridHdr *qhdr;  /* [kVerifyProblemsPerLaunch] */
    size_t Pn;         /* FineWork's */
};
/* n <= kVerifyProblemsPerLaunch matches; w: the voxel clouds (vox, vox_n, Pn); results: the call's d_results (T is read) */
void launch_verify_move(const VerifyProblem *probs, int n, const FineWork &w, const bev_icp_result_t *results, const VerifyTarget &t,
                        const VerifyWork &v, bev_verify_result_t *out, hipStream_t st);
/* both directions of the same matches; slices: workgroups of `slice` points over the largest cloud of either side */
void launch_verify_count(const VerifyProblem *probs, int n, uint32_t slices, const FineWork &w, const VerifyTarget &t,
                         const VerifyWork &v, const bev_verify_params_t &prm, uint32_t slice, bev_verify_result_t *out, hipStream_t st);

/* ---- translation guess of retrieved pairs: height-grid offset search (bev_align.h) ---- */
struct AlignShape { /* bev_align_params_t as the kernels take it, and what a point's value needs */
    int G, S, K, skip_label0;
    float cell, yaw_step, lidar_to_ground;
};
/* a hit as it goes up: the query's records, the candidate's grid (-1: none, read as an empty grid) and the yaw */
struct AlignHit {
    uint64_t off;
    uint32_t n;
    int32_t cand;
    float angle_guess;
    uint32_t _pad;
};
static_assert(sizeof(AlignHit) == 24, "the device reads this layout");
/* what k_align_hit leaves of one (hit, flip, k) hypothesis: its best shift, the query grid's sum of squares and the scores of
 * the shift's four neighbours (0 where a neighbour lies outside the window: not read then) */
struct AlignHyp {
    uint32_t score;
    int32_t dx, dy;
    uint32_t eq, sxm, sxp, sym, syp;
};
static_assert(sizeof(AlignHyp) == 32, "one record per hypothesis");
/* the words of dynamic LDS of k_align_hit for a shape: the plane of G * G words, then the packed query, the padded candidate,
 * the table of scores and the reduction's scratch in its place */
size_t align_hit_lds_bytes(const AlignShape &as);
/* rows, ent0, blocks and entries as for launch_place_splat; planes: G * G words per grid, zeroed by the caller on the stream */
void launch_align_grid(const bev_point_t *clouds, const void *rows, const uint32_t *ent0, int nf, uint32_t blocks,
                       const void *entries, const AlignShape &as, uint32_t *planes, hipStream_t st);
/* n_grids planes into grids (G * G bytes each) and energy (their sums of squares) */
void launch_align_finish(const uint32_t *planes, int n_grids, const AlignShape &as, uint8_t *grids, uint32_t *energy, hipStream_t st);
/* n hits from hits[0]: hyp[(h * 2 + flip) * (2K + 1) + (k + K)] */
void launch_align_hit(const bev_point_t *clouds, const AlignHit *hits, int n, const uint8_t *grids, const AlignShape &as,
                      AlignHyp *hyp, hipStream_t st);
/* ... and their results[2h + flip], best[h] and (where wanted) detail[2h + flip] */
void launch_align_pick(const AlignHit *hits, int n, const AlignHyp *hyp, const uint32_t *energy, const AlignShape &as,
                       bev_icp_result_t *results, int32_t *best, bev_align_detail_t *detail, hipStream_t st);

/* opt in to > 64 KiB of dynamic LDS for the kernels that need it */
hipError_t configure_kernels(const Geometry &g);
size_t cell_sums_lds_bytes();
size_t raster_lds_bytes(const Geometry &g);

} /* namespace bevk */
#endif
