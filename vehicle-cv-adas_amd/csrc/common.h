// common.h -- error plumbing shared by the C-ABI translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include "../../include/adas_hip.h"

namespace adas {
void set_error(const char* fmt, ...);
int hip_fail(hipError_t e, const char* what, const char* file, int line);
// Parameters that a captured pipeline step bakes into its kernel arguments (post / decode / geometry configuration) carry a
// process-wide generation: every setter bumps it, adas_pipeline_* re-captures when it moved since the capture.
inline bool env_on(const char* name) {   // an environment switch: set to 1 (ADAS_NO_STEM=1)
    const char* v = getenv(name);
    return v && v[0] == '1';
}
unsigned long long config_generation();
void bump_config_generation();
}  // namespace adas

// frames a post-processing handle was created for (post_kernels.hip): adas_pipeline_create checks them against n_streams x micro_batch
struct adas_yolo_post;
struct adas_ufld_decode;
struct adas_lane_geometry;
struct adas_birdview;
struct adas_warp;
struct adas_analysis;
struct adas_bytetrack;
namespace adas {
int handle_max_batch(const ::adas_yolo_post* h);
int handle_max_batch(const ::adas_ufld_decode* h);
int handle_max_batch(const ::adas_lane_geometry* h);
// the decoder's device arrays (post_kernels.hip): counts [B][4], detected [B][4], points [B][4][128][2]
void decode_lane_views(const ::adas_ufld_decode* h, const int** cnt, const int** det, const int** pts);
// what adas_pipeline_attach_birdview checks (birdview_kernels.hip, warp_kernels.hip); 0 for a null handle
int birdview_capacity(const ::adas_birdview* h, int* n_streams, int* max_frames);
int warp_geometry(const ::adas_warp* h, int* src_h, int* src_w, int* max_batch);
// the bird view's pending-request table, [n_streams] words (birdview_kernels.hip): the analysis stage stores each stream's next request there
int* birdview_request_table(::adas_birdview* h);
// what adas_pipeline_attach_analysis checks and does (analysis_kernels.hip): the handle's capacity; bind = remember the bird view whose
// requests the handle now owns and queue every stream's initial "Default" on hip_stream (bird may be null: unbind)
int analysis_capacity(const ::adas_analysis* h, int* n_streams, int* max_frames);
int analysis_bind_birdview(::adas_analysis* h, ::adas_birdview* bird, int n_streams, void* hip_stream);
}  // namespace adas
// what the overlay stage reads of the other handles (overlay_kernels.hip) and what adas_pipeline_attach_overlay checks
struct adas_overlay;
namespace adas {
int decode_num_lanes(const ::adas_ufld_decode* h);                       // lanes of the decoded tensors (4 for UFLD v1)
const int* geometry_bird_points(const ::adas_lane_geometry* h);         // [B][4][128][2]; the counts are header words 4..7
// the analysis handle's frame records (int32 words, `stride` words apart) and distance points [max_frames][max_points][2]
void analysis_frame_views(const ::adas_analysis* h, const int** frames, int* stride, const int** pts_xy, int* max_points);
void warp_dst_geometry(const ::adas_warp* h, int* dst_h, int* dst_w);
int overlay_geometry(const ::adas_overlay* h, int* src_h, int* src_w, int* bird_h, int* bird_w, int* max_batch);
// what the overlay's object layer reads (post_kernels.hip): the survivors as RectInfo.tolist() corners [B][cap][4] with classes [B][cap] and
// counts [B][4] (n_keep is word 2); the tracker's live table, stream s at + s * stream_bytes: its header, and its rows in the layout of
// adas_track, the tracked list first and in list order
void post_survivor_views(const ::adas_yolo_post* h, const int** xyxy_int, const int** cls, const int** counts, int* cap);
void tracker_live_views(const ::adas_bytetrack* h, const unsigned char** hdr, const unsigned char** out, size_t* stream_bytes, int* n_streams,
                        int* max_tracks);
// the trajectory rings behind the live table (post_kernels.hip), stream s at + s * stream_bytes: the tracked list's slot ids [max_tracks] int,
// the first slot's count of boxes ever appended (the next slot's slot_bytes further on), and the rings [max_tracks][30][4] fp64 by slot,
// entry i of a track's list at i % 30
void tracker_ring_views(const ::adas_bytetrack* h, const unsigned char** tracked_slots, const unsigned char** appended, size_t* slot_bytes,
                        const unsigned char** rings);
// room for the records of det_cap + trk_cap boxes per frame, ahead of a captured step (overlay_kernels.hip)
int overlay_reserve_objects(::adas_overlay* h, int det_cap, int trk_cap);
// the same for the trajectories stage: the primitives of trk_cap tracks per frame and the stage's plane
int overlay_reserve_trajectories(::adas_overlay* h, int trk_cap);
// one overlay run from the handles' device arrays (overlay_kernels.hip): the arguments of adas_overlay_run_trajectories behind the handle, in
// its order; a handle whose stages are off may be null.  who names the caller in messages, mask is the stage bits it accepts.  The public
// adas_overlay_run* entry points and the pipeline's step all go through it
struct overlay_handles {
    const uint8_t* d_src_bgr;
    uint8_t* d_dst_bgr;
    const ::adas_ufld_decode* decode;
    ::adas_lane_geometry* geometry;
    ::adas_analysis* analysis;
    ::adas_yolo_post* post;
    ::adas_bytetrack* tracker;
    uint8_t* d_bird_bgr;
    int stages, n_streams, n_frames;
    void* stream;
};
int overlay_run_handles(const char* who, int mask, ::adas_overlay* h, const overlay_handles& a);
// the UI panels (overlay_panels.hip) keep their state -- geometry, sprite atlas, latches, records -- behind one pointer of the overlay handle
// (overlay_kernels.hip: overlay_panel_slot; adas_overlay_destroy frees it through overlay_panels_free).  overlay_own_frames: the handle's own
// buffer and how many of its frames some run has written; overlay_note_stream: the stream the fetches drain.  overlay_run_panels: the run of
// adas_overlay_run_panels under the caller's name (the pipeline's step); overlay_panels_ready: adas_overlay_set_panels has been called
struct overlay_panels;
overlay_panels** overlay_panel_slot(::adas_overlay* h);
void overlay_panels_free(overlay_panels* s);
int overlay_own_frames(::adas_overlay* h, uint8_t** d_bgr, int* frames_written);
void overlay_note_stream(::adas_overlay* h, void* stream);
bool overlay_panels_ready(::adas_overlay* h);
int overlay_run_panels(const char* who, ::adas_overlay* h, uint8_t* d_frames_bgr, const ::adas_analysis* analysis, const uint8_t* d_bird_bgr, int panels,
                       int n_streams, int n_frames, void* stream);
// the text (overlay_text.hip) keeps its state -- fonts, style, class names, caller lines, item lists -- behind one pointer of the overlay handle too
// (overlay_text_slot; adas_overlay_destroy frees it through overlay_text_free).  overlay_class_colors: the packed class colours of the object
// layer (which: 0 detections, 1 tracks), the colours the labels and ids are drawn in
struct overlay_text;
overlay_text** overlay_text_slot(::adas_overlay* h);
void overlay_text_free(overlay_text* s);
void overlay_class_colors(const ::adas_overlay* h, int which, const uint32_t** table, int* n);
// overlay_run_text: the run of adas_overlay_run_text under the caller's name -- the layout of `mask`, then the draw of its kinds in draw_now;
// overlay_draw_text: the kinds `sources` of that layout, painted later on the handle's own buffer (the pipeline's step paints the panel
// strings and the lines behind the panels); overlay_text_ready: a font has been set.  analysis_points_d: the metres of the analysis
// handle's distance points [max_frames][max_points], beside analysis_frame_views' pts_xy
bool overlay_text_ready(::adas_overlay* h);
int overlay_run_text(const char* who, ::adas_overlay* h, uint8_t* d_frames_bgr, const ::adas_yolo_post* post, const ::adas_bytetrack* tracker,
                     const ::adas_analysis* analysis, int mask, int draw_now, int n_streams, int n_frames, void* stream);
int overlay_draw_text(const char* who, ::adas_overlay* h, int sources, int n_frames_total, void* stream);
const double* analysis_points_d(const ::adas_analysis* h);
// the bird view's readouts (overlay_readout.hip) keep their state -- style, half-width table, per-frame records -- behind one pointer of the
// overlay handle as well (overlay_readout_slot; adas_overlay_destroy frees it through overlay_readout_free).  geometry_veh_pos: the geometry
// handle's veh_pos array [B] (post_kernels.hip).  overlay_text_font_tables: the text state's font table on the device and its host copy
// (TextFont[ADAS_TEXT_FONTS]; nulls while no font is set).  overlay_readout_sources: what frame q of a run reads -- direction at
// dir[q * dir_stride], veh_pos at veh[q], curvature and offset at cur[q * val_stride] / off[q * val_stride].  overlay_readout_check: the
// refusals of a run with the stage, under the caller's name; overlay_readout_launch: its two launches, in place on d_bird
// [frames][bird_h][bird_w][3]; overlay_readout_reserve: the state, ahead of a captured step
struct overlay_readout;
overlay_readout** overlay_readout_slot(::adas_overlay* h);
void overlay_readout_free(overlay_readout* s);
const double* geometry_veh_pos(const ::adas_lane_geometry* h);
void overlay_text_font_tables(::adas_overlay* h, const void** d_fonts, const void** h_fonts);
struct overlay_readout_sources {
    const int32_t* dir;
    const double *veh, *cur, *off;
    int dir_stride, val_stride;
};
int overlay_readout_reserve(::adas_overlay* h);
int overlay_readout_check(const char* who, ::adas_overlay* h);
int overlay_readout_launch(::adas_overlay* h, const overlay_readout_sources& s, uint8_t* d_bird, int frames, void* stream);
}  // namespace adas
// what adas_pipeline_attach_jpeg checks (jpeg_kernels.hip); zeros for a null handle
struct adas_jpeg;
namespace adas {
void jpeg_geometry_of(const ::adas_jpeg* h, int* width, int* height, int* max_batch);
}  // namespace adas
// what adas_pipeline_attach_jpegdec checks and adas_pipeline_step_jpeg_host drives (jpegdec_kernels.hip): the handle's geometry (zeros for a
// null handle) and own frame buffer; jpegdec_stage_host packs host streams into the handle's next staging slot and queues the copy on
// copy_stream, jpegdec_run_slot decodes that slot on `stream` (the two halves of adas_jpegdec_run_host)
struct adas_jpegdec;
namespace adas {
void jpegdec_geometry_of(const ::adas_jpegdec* h, int* width, int* height, int* max_batch);
uint8_t* jpegdec_frames(::adas_jpegdec* h);
int jpegdec_next_slot(const ::adas_jpegdec* h);   // the staging slot (0 or 1) the next jpegdec_stage_host packs into
int jpegdec_stage_host(::adas_jpegdec* h, const uint8_t* const* h_streams, const int64_t* h_lengths, int batch, void* copy_stream, int* slot);
int jpegdec_run_slot(::adas_jpegdec* h, int slot, int batch, uint8_t* d_dst_bgr, void* stream);
}  // namespace adas

// what adas_pipeline_attach_yuv checks and adas_pipeline_step_yuv* use (yuv_kernels.hip): the handle's geometry and frame_stride (zeros for a
// null handle) and its own BGR frames
struct adas_yuv;
namespace adas {
void yuv_geometry_of(const ::adas_yuv* h, int* width, int* height, int* max_batch, long long* src_bytes);
uint8_t* yuv_frames(::adas_yuv* h);
long long yuv_extent_of(const ::adas_yuv* h);   // bytes of a source frame that are read (adas_yuv_frame_bytes)
}  // namespace adas
// what adas_pipeline_attach_yuvout checks (yuvout_kernels.hip); zeros for a null handle
struct adas_yuvout;
namespace adas {
void yuvout_geometry_of(const ::adas_yuvout* h, int* width, int* height, int* max_batch);
}  // namespace adas
// what adas_pipeline_attach_scale and its two consumers check (scale_kernels.hip); zeros for a null handle
struct adas_scale;
namespace adas {
void scale_geometry_of(const ::adas_scale* h, int* src_w, int* src_h, int* canvas_w, int* canvas_h, int* tiles, int* max_batch, int* border);
}  // namespace adas
// what adas_pipeline_attach_remap checks and adas_pipeline_step_frames uses (remap_kernels.hip): the handle's geometry (zeros for a null
// handle) and its own BGR frames (null until the handle has touched the device)
struct adas_remap;
namespace adas {
void remap_geometry_of(const ::adas_remap* h, int* src_h, int* src_w, int* dst_h, int* dst_w, int* n_streams, int* max_batch);
uint8_t* remap_frames(::adas_remap* h);
void remap_forget_stream(::adas_remap* h);   // the handle's last run has drained and its stream goes away: later calls use the null stream
}  // namespace adas

#define ADAS_HIP_TRY(expr)                                                     \
    do {                                                                        \
        hipError_t e__ = (expr);                                                \
        if (e__ != hipSuccess) return adas::hip_fail(e__, #expr, __FILE__, __LINE__); \
    } while (0)

#define ADAS_REQUIRE(cond, code, ...)      \
    do {                                   \
        if (!(cond)) {                     \
            adas::set_error(__VA_ARGS__);  \
            return (code);                 \
        }                                  \
    } while (0)
