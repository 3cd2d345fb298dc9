// Host launchers of the gfx950 kernels (definitions in the .hip files).
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "common.h"

namespace pr {
void launch_calib_basic(const FramePtrs& fp, int nframes, uint64_t ped, uint64_t gf, int64_t npix, int kind,
                        uint64_t stream);
void launch_calib_image(const FramePtrs& fp, int nframes, uint64_t ped, uint64_t gf, int64_t npix, int kind,
                        uint64_t idx, int64_t nout, uint64_t stream);
void launch_calib_cm(const FramePtrs& fp, int nframes, uint64_t ped, uint64_t gf, uint64_t elig, int kind,
                     int n_panels, int panel_rows, int panel_cols, int asic_rows, int asic_cols, float thr,
                     float maxcorr, int npix_min, int flags, int bank_cols, uint64_t stream,
                     uint64_t img_desc = 0, uint64_t gap_runs = 0,
                     int n_gap_runs = 0,    // img_desc: fused K-05 (ImgOut); gap runs zeroed by the same kernel
                     uint64_t ped_sg = 0,   // signed pedestal tables (eligibility in the sign bits), 0 = planes
                     uint64_t plain_mask = 0);  // bit f: plain (not streaming) stores for frame f
size_t cm_lds_bytes(int asic_rows, int asic_cols, int kind);
bool cm_signed_shape(int kind, int asic_rows, int asic_cols, int bank_cols);   // reads signed pedestal tables
void launch_image_tiles(const FramePtrs& fp, int nframes, bool calib, int kind, uint64_t ped, uint64_t gf,
                        int64_t npix, int panel_rows, int panel_cols, uint64_t tiles, int n_tiles, int tiles_x,
                        uint64_t codes, int img_h, int img_w, uint64_t stream);
int image_tile_h();
int image_tile_w();
int image_tile_stage();
int cm_tile_cols(int asic_rows, int asic_cols, int bank_cols, int max_cols, int kind);
void launch_convert_u16_f32(const FramePtrs& fp, int nframes, int64_t npix, uint64_t stream);
void launch_read_f32(const FramePtrs& fp, int nframes, int64_t npix, int k, bool nt, uint64_t sums, uint64_t stream);
void launch_xor_selftest(uint64_t out, uint64_t stream);
// diagnostic builds only (-DPR_CM_STAMPS=1): per-wave phase stamps of the epix10k2M CM kernel
void cm_set_stamp_buffer(uint64_t p);
void launch_fill_runs(const FramePtrs& fp, int nframes, uint64_t runs, int n_runs, uint64_t stream);
void launch_mask_frames(const FramePtrs& fp, int nframes, uint64_t zero, int64_t npix, uint64_t stream);
void launch_gather_frames(const FramePtrs& fp, int nframes, int64_t nelem, bool bf16, uint64_t stream);
// host (pinned / registered) -> HBM copy by a kernel; false = not applicable, use hipMemcpyAsync
bool launch_copy_h2d(uint64_t dst, uint64_t host_src, int64_t bytes, int workgroups, uint64_t stream);
// device -> device (incl. IPC-mapped peer HBM) copies of up to kMaxCopyRuns runs in ONE launch
// (queue fabric); fills cr.cstart, returns the grid size used
int launch_copy_runs(CopyRuns& cr, int workgroups, uint64_t stream);
void launch_assemble(const FramePtrs& fp, int nframes, uint64_t idx, int64_t nout, uint64_t omask,
                     uint64_t stream);
// scratch: 0, or a zero-initialised PfScratch block (kPfScratchBytes) reused by every launch on one
// stream: counts / summary then need no zeroing before the launch (csrc/peakfind.hip)
// The block also holds each workgroup's candidate SPILL list (hit-rich frames): candidates beyond the
// kPfCandCap parked in LDS go to the workgroup's kPfSpillCap entries here and are tested after the
// stream like the parked ones (only past both does a candidate get tested inline in the stream).
constexpr int kPfScratchHeader = 1024;                 // PfScratch (counters), padded
// The grid is one resident wave of workgroups (768 for radius 1, 512 for radius 2 on 256 CUs), so
// 1024 lists of 4096 entries cover every workgroup with 4x the round-3 depth: on a 2 %-candidate
// batch the in-stream path no longer runs (11.2 -> 7.4 us/frame, profiles/r4/README.md section 4).
#ifndef PR_PF_SPILL_WGS
#define PR_PF_SPILL_WGS 1024
#endif
constexpr int kPfSpillWgs = PR_PF_SPILL_WGS;                    // workgroups with a spill list
constexpr int kPfSpillCap = (4096 / kPfSpillWgs) * 1024;        // entries each (same block size)
constexpr int64_t kPfScratchBytes = kPfScratchHeader + (int64_t)kPfSpillWgs * kPfSpillCap * 4;
void launch_peakfind(const FramePtrs& fp, int nframes, int n_panels, int rows, int cols, float thr_peak,
                     float son_min, int radius, int max_peaks, uint64_t peaks, uint64_t counts,
                     uint64_t summary, uint64_t total, uint64_t stream,
                     uint64_t scratch = 0);
// K-08 radial profile (csrc/radial.hip): per-frame int64 sums / int32 counts [F, nbins], float32
// profiles [F, nbins] and, when run != 0, the run accumulator int64 [2 * nbins + 1] (run_sum,
// run_count, frames).  bins: uint16 [n], 0xFFFF = excluded, every other entry < nbins (the caller
// validates the map; the kernel ignores entries >= nbins).  Clears sums / counts on the stream first.
constexpr int kRadMaxBins = 4096;
void launch_radial(const FramePtrs& fp, int nframes, int64_t n, uint64_t bins, int nbins, float vmin, float vmax,
                   int frac_bits, uint64_t sums, uint64_t counts, uint64_t profile, uint64_t run, uint64_t stream);
// K-09 dark statistics (csrc/dark.hip): ADDS up to kMaxFrames raw uint16 frames of n elements into
// cnt int32 [NC, n], sum int64 [NC, n], sq int64 [NC, n] (NC = 2 / 3 / 1 for kind epix10ka / jungfrau /
// plain): valid samples with adu_lo <= adu <= adu_hi.  Never clears; one owner thread per pixel, so
// two launches in flight must not share accumulators.
void launch_dark(const FramePtrs& fp, int nframes, int64_t n, int kind, int adu_lo, int adu_hi, uint64_t cnt,
                 uint64_t sum, uint64_t sq, uint64_t stream);
// K-10 zero suppression (csrc/sparse.hip): the pixels of up to kMaxFrames float32 frames of n elements
// with thr <= v <= vmax (and mask[i] != 0 when mask != 0), as (index, value) pairs packed frame after
// frame in index order.  nnz int32 [F], flags uint8 [F] (bit 0 overflow, bit 1 skipped), offs int64
// [F + 1], pix int32 / val float32 [>= F * cap].  keys (int32 [F] on the device, or 0): frame f is
// skipped unless keys[f] >= key_min.  scratch: a 16-B aligned block of at least
// sparsify_scratch_bytes(n, cap, F) bytes, owned by one stream; the launch clears what it needs.
constexpr int kSparseChunk = 4096;          // elements per scan chunk (one directory entry each)
constexpr int kSparseScratchHeader = 256;   // the frames' cursors
int64_t sparsify_scratch_bytes(int64_t n, int64_t cap, int frames);
void launch_sparsify(const FramePtrs& fp, int nframes, int64_t n, float thr, float vmax, int64_t cap, uint64_t mask,
                     uint64_t keys, int key_min, uint64_t nnz, uint64_t flags, uint64_t offs, uint64_t pix,
                     uint64_t val, uint64_t scratch, int64_t scratch_bytes, uint64_t stream,
                     int phases = 3);   // measurements only: 1 = clear + scan, 2 = pack of a block just scanned
// K-11 powder statistics (csrc/powder.hip): ADDS up to kMaxFrames float32 frames of n elements into the
// planar accumulators cnt int32 / sum int64 / sq int64 / qmax int32 / above int32 [nc, n] and nfr int64
// [nc]: samples with vmin <= v <= vmax, quantised as q = rintf(v * 2^frac_bits).  nc == 2: keys (int32
// [F] on the device) puts frame f into class 1 iff keys[f] >= key_min; nc == 1: keys == 0.  Never
// clears (the caller sets qmax to INT32_MIN once); one owner thread per pixel, so two launches in
// flight must not share accumulators.
void launch_powder(const FramePtrs& fp, int nframes, int64_t n, float vmin, float vmax, int frac_bits,
                   float thr_above, int nc, uint64_t keys, int key_min, uint64_t nfr, uint64_t cnt, uint64_t sum,
                   uint64_t sq, uint64_t qmax, uint64_t above, uint64_t stream);
// K-12 per-pixel histograms (csrc/pixhist.hip): ADDS up to kMaxFrames float32 frames of n elements into
// hist int32 [n, nbins] (pixel-major): a sample with lo <= v <= hi adds 1 to bin min(nbins - 1,
// (int) floorf((v - lo) * inv_w)), inv_w = float32(nbins / (hi - lo)) from the caller.  n * nbins < 2^31.
// Never clears; one owner workgroup per pixel, so two launches in flight must not share an accumulator.
// pixel_hist_tile_pixels: the consecutive pixels one workgroup owns (a power of two, 64 .. 1024).
constexpr int kHistMaxBins = 1024;
int pixel_hist_tile_pixels(int nbins);
void launch_pixel_hist(const FramePtrs& fp, int nframes, int64_t n, float lo, float hi, float inv_w, int nbins,
                       uint64_t hist, uint64_t stream,
                       int layout = 0);   // measurements only: 1 = word-major LDS tile, 2 = unpadded row pitch
// K-13 photon counting (csrc/photons.hip): up to kMaxFrames float32 frames of shape [P, H, W] -> photons per
// pixel k (whole photons by floor of v * inv, plus one where a seed's remainder and its largest 4-connected
// neighbour remainder of the same panel reach thr_total).  ADDS to the planar run accumulators cnt int32 /
// psum int64 / occ int32 [n] (never clears; one owner lane per pixel, so two launches in flight must not
// share a set); clears on the stream, then fills pk int32 [F, n_roi, 8] and tot int64 [F, n_roi]; writes
// kmap uint8 [F, n] when kmap != 0.  mask uint8 [n] (0 = all kept), roi uint8 [n] labels (0 = one ROI).
// inv = float32(1 / adu_per_photon) from the caller.  photons_block_pixels: the consecutive pixels one block
// of lanes owns (a lane owns photons_lane_pixels: 4 when W % 4 == 0, else 1); a workgroup owns several blocks
// once there are more than photons_max_grid of them.
int photons_lane_pixels(int W);
int photons_block_pixels(int W);
int photons_max_grid();
void launch_photons(const FramePtrs& fp, int nframes, int P, int H, int W, float inv, float vmax, float thr_seed,
                    float thr_total, uint64_t mask, uint64_t roi, int n_roi, uint64_t kmap, uint64_t cnt,
                    uint64_t psum, uint64_t occ, uint64_t pk, uint64_t tot, uint64_t stream,
                    int variant = 0);   // measurements only: bit 0 = 2 frames in flight, bits 8.. = grid cap
// K-14 droplets (csrc/droplets.hip): the 4-connected clusters of the pixels of up to kMaxFrames float32 frames
// of shape [P, H, W] that the mask keeps and whose value lies in [thr_low, vmax], kept when a pixel reaches
// thr_seed.  Writes nact / ndrop int32 [F], flags uint8 [F] (bit 0 = ndrop > cap, bit 2 = nact > cap_pix; either
// stores nothing), offs int64 [F + 1] and the columns label / npix / qmax int32, adu / sy / sx int64 of F * cap
// rows: frame f's droplets at offs[f] .. offs[f + 1], label ascending.  The first launch is K-10's scan and
// pack (launch_sparsify) into the scratch block of droplets_scratch_bytes(n, cap_pix, cap, F) bytes, owned by
// one stream; no launch after it reads a frame.  One call is complete in itself: nothing needs clearing.
int64_t droplets_scratch_bytes(int64_t n, int64_t cap_pix, int64_t cap, int frames);
void launch_droplets(const FramePtrs& fp, int nframes, int P, int H, int W, float thr_low, float thr_seed, float vmax,
                     int frac_bits, int64_t cap_pix, int64_t cap, uint64_t mask, uint64_t nact, uint64_t ndrop,
                     uint64_t flags, uint64_t offs, uint64_t label, uint64_t npix, uint64_t adu, uint64_t sy, uint64_t sx,
                     uint64_t qmax, uint64_t scratch, int64_t scratch_bytes, uint64_t stream,
                     int phases = 15);   // measurements only: 1 = scan, 2 = index + link, 4 = reduce, 8 = count + pack
// K-15 cube (csrc/cube.hip): ADDS up to kMaxFrames float32 frames of n elements into the planar accumulators
// cnt int32 / sum int64 / sq int64 [nbins, n] and nfr int64 [nbins], frame f into plane bins[f]: samples with
// vmin <= v <= vmax, quantised as q = rintf(v * 2^frac_bits).  bins is a HOST array of nframes int32 in
// -1 .. nbins - 1; a frame with bin -1 is dropped (not read), a bin without a frame in the launch is neither
// read nor written, and nothing is launched when every frame is dropped.  Never clears; one owner thread per
// pixel, so two launches in flight must not share accumulators.
constexpr int kCubeMaxBins = 4096;
void launch_cube(const FramePtrs& fp, int nframes, int64_t n, float vmin, float vmax, int frac_bits, int nbins,
                 const int32_t* bins, uint64_t nfr, uint64_t cnt, uint64_t sum, uint64_t sq, uint64_t stream);
// K-16 ROI statistics (csrc/roi.hip): per frame and rectangle of up to kMaxFrames float32 frames of shape
// [P, H, W] the row of eight 64-bit words npix, sum q, sum q * y, sum q * x, key, 0, 0, 0 over the pixels
// with vmin <= v <= vmax that the mask (uint8 [n], 0 = all kept) keeps, q = rintf(v * 2^frac_bits); key packs
// the largest q and the lowest index that attains it (0 = no sample).  rows: uint64 [F, R, 8], 64-B aligned;
// projx int64 [F, Lx] / projy int64 [F, Ly] (0 = not wanted): the rectangles' column / row sums, one after
// the other.  Clears all three for its F frames on the stream first, and touches nothing beyond them.
// RoiPlan: the rectangles (p, y0, y1, x0, x1; half-open, at most kRoiMaxRects, overlaps allowed) cut into
// strips of roi_strip_rows(width) rows, one per workgroup; built once per run, it owns its device copy.
constexpr int kRoiMaxRects = 16;
int roi_strip_rows(int width);
// tests and measurements only: force 1 or 2 row iterations' loads in flight (0 = by the grid's size, the default;
// -1 = only return the setting)
int roi_rows_ahead(int set = -1);
int roi_strip_pixels(int set = 0);   // measurements only: another strip size for the plans built from now on; returns it
// the strips of a plan as the kernel reads them, 8 int32 words each: r, p * H + y, rows, x0, x1, y, offx, offy + dy
std::vector<int32_t> roi_plan_strips(const std::vector<int32_t>& rects, int P, int H, int W);
struct RoiPlan {
  RoiPlan(const std::vector<int32_t>& rects, int P, int H, int W, int device);
  ~RoiPlan();
  RoiPlan(const RoiPlan&) = delete;
  RoiPlan& operator=(const RoiPlan&) = delete;
  int P, H, W, device;
  int R = 0, nstrips = 0;
  int64_t Lx = 0, Ly = 0;
  std::vector<int32_t> rects;
  uint64_t strips = 0;   // RoiStrip [nstrips] on the device
};
void launch_roi(const FramePtrs& fp, int nframes, const RoiPlan& plan, float vmin, float vmax, int frac_bits,
                uint64_t mask, uint64_t rows, uint64_t projx, uint64_t projy, uint64_t stream);
// K-17 roibin (csrc/roibin.hip): of up to kMaxFrames float32 frames of shape [P, H, W], given the peak finder's
// peaks float32 [F, max_peaks, 8] and counts int32 [F] on the device, every frame with counts[f] >= min_peaks
// as codes int16 [F, P, Hb, Wb] (the B x B block means of q = rintf(v * inv) over the pixels with vmin <= v <=
// vmax that the mask keeps, rounded half up, clamped to +-32767, -32768 = no pixel) and one box per valid
// record, ordered by centre: ctr int32, rec uint32 [.., 8], box uint32 [.., 2R+1, 2R+1] of F * max_peaks rows,
// frame f's at offs[f] .. offs[f + 1] (offs int64 [F + 1]).  npk / nbox / nbad / nsat int32 [F], flags uint8 [F]
// (bit 0 = more peaks than max_peaks: no boxes, bit 1 = skipped, bit 2 = an invalid record).  A skipped frame is
// not read and its code rows are not written.  One call is complete in itself: nothing needs clearing.
constexpr int kRoibinMaxPeaks = 4096;   // the sort keys of a frame fit LDS
constexpr int kRoibinMaxRadius = 7;
void launch_roibin(const FramePtrs& fp, int nframes, int P, int H, int W, int B, float inv, float vmin, float vmax,
                   int R, int min_peaks, int max_peaks, uint64_t mask, uint64_t peaks, uint64_t counts, uint64_t codes,
                   uint64_t npk, uint64_t nbox, uint64_t nbad, uint64_t nsat, uint64_t flags, uint64_t offs,
                   uint64_t ctr, uint64_t rec, uint64_t box, uint64_t stream,
                   int phases = 3);   // measurements only: 1 = headers + codes, 2 = boxes of a batch just binned
}  // namespace pr
