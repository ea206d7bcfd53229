// pipeline.cpp -- the fused per-frame ADAS step (detector + NMS, lane + decode, tracker) for
// n_streams independent video streams, optionally replayed from a hipGraph.
// Mirrors what demo.py:261-281 drives per frame, minus UI; nothing returns to the host per step.
#include "engine.h"
#include <stdlib.h>

struct adas_yolo_post;
struct adas_ufld_decode;
struct adas_bytetrack;

struct adas_pipeline {
    adas_pipeline_desc d;
    // optional stages behind the lane decode (adas_pipeline_attach_birdview): per-stream adaptive homographies, and the bird-view image
    adas_birdview* bird = nullptr;
    adas_warp* bird_warp = nullptr;
    // optional last stage behind the join of the two branches (adas_pipeline_attach_analysis): distance, collision and warning state
    adas_analysis* analysis = nullptr;
    // optional drawing stage behind it (adas_pipeline_attach_overlay): discs, area polygon and alpha blends into the overlay handle's buffer
    adas_overlay* overlay = nullptr;
    int overlay_stages = -1;   // ADAS_OVERLAY_*; -1: everything the attached handles allow
    int overlay_panels = 0;    // ADAS_PANEL_* painted behind the overlay's run (adas_pipeline_set_overlay_panels); 0: none
    int overlay_text = 0;      // ADAS_TEXT_* painted over the overlay's frames (adas_pipeline_set_overlay_text); 0: none
    int overlay_readouts = 0;  // ADAS_OVERLAY_READOUTS or 0 (adas_pipeline_set_overlay_readouts): the bird view's arrows and strings
    // optional encoding stage, the step's last launch group (adas_pipeline_attach_jpeg): one baseline JPEG stream per frame
    adas_jpeg* jpeg = nullptr;
    int jpeg_source = ADAS_JPEG_SRC_OVERLAY;
    // optional raw-video stage behind the overlay (adas_pipeline_attach_yuvout): every frame as NV12 / NV21 / I420 / YUYV / UYVY
    adas_yuvout* yuvout = nullptr;
    int yuvout_source = ADAS_YUVOUT_SRC_OVERLAY;
    // optional scaling stage behind the overlay (adas_pipeline_attach_scale): every frame a tile of a canvas, and the canvases' own encoders
    adas_scale* scale = nullptr;
    int scale_source = ADAS_SCALE_SRC_OVERLAY;
    adas_jpeg* scale_jpeg = nullptr;
    adas_yuvout* scale_yuvout = nullptr;
    hipStream_t st = nullptr;
    hipStream_t st_lane = nullptr;  // graph mode: the lane branch is captured on its own stream so the two nets overlap
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // A captured step bakes every kernel argument in: the input pointers, the source geometry, the lane crop ratio and the
    // post / decode / geometry configuration (the latter through adas::config_generation()).  All of them are the cache key.
    struct GraphKey {
        const void* in_a;   // detector seam tensor, or the u8 frames
        const void* in_b;   // lane seam tensor (null for a step_frames entry)
        int src_h, src_w;   // step_frames: camera geometry (0 for a seam-tensor entry)
        double crop;        // step_frames: lane crop ratio
        bool operator==(const GraphKey& o) const {
            return in_a == o.in_a && in_b == o.in_b && src_h == o.src_h && src_w == o.src_w && crop == o.crop;
        }
    };
    struct Cached {
        GraphKey key;
        hipGraph_t graph;
        hipGraphExec_t exec;
    };
    std::vector<Cached> graphs;              // one captured step per distinct key
    hipGraph_t last_graph = nullptr;         // the capture the last graph-mode step replayed (adas_pipeline_graph_kernels)
    unsigned long long graphs_gen = 0;       // config generation the cached captures were recorded under
    hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool timed = false;
    bool sink = false;   // the detector's fused v8 Detect feeds the post-processing's scan arrays directly (decided at create)
    // step_frames: u8 camera frames in, the engine-seam tensors live here
    float* det_in = nullptr;
    float* lane_in = nullptr;
    struct FrameSrc {
        const uint8_t* frames;
        int h, w;
        double crop;
    };
    FrameSrc fsrc{nullptr, 0, 0, 0.0};  // set while a step_frames call records
    bool packed = false;  // both first layers are the fused stem: the seam tensors are (c0,c1,c2,0) 16-bit NHWC, 8 B per pixel
    // step_frames_host: two device frame buffers filled by a copy stream
    hipStream_t st_copy = nullptr;
    uint8_t* host_stage[2] = {nullptr, nullptr};
    size_t host_stage_bytes = 0;
    hipEvent_t ev_copied[2] = {nullptr, nullptr}, ev_consumed[2] = {nullptr, nullptr};
    unsigned long long host_steps = 0;
    // step_jpeg_host: the decoder in front of the step (adas_pipeline_attach_jpegdec); its two staging slots are filled by the copy stream
    adas_jpegdec* jpegdec = nullptr;
    hipEvent_t ev_jcopied[2] = {nullptr, nullptr}, ev_jconsumed[2] = {nullptr, nullptr};
    bool jslot_used[2] = {false, false};
    // step_yuv / step_yuv_host: the conversion in front of the step (adas_pipeline_attach_yuv); the raw frames of a host step go through two
    // device buffers filled by the copy stream, as step_frames_host's do
    adas_yuv* yuv = nullptr;
    uint8_t* yuv_stage[2] = {nullptr, nullptr};
    size_t yuv_stage_bytes = 0;
    hipEvent_t ev_ycopied[2] = {nullptr, nullptr}, ev_yconsumed[2] = {nullptr, nullptr};
    unsigned long long yuv_steps = 0;
    // step_frames: the rectification in front of the step (adas_pipeline_attach_remap), behind every way in; the step reads the handle's frames
    adas_remap* remap = nullptr;
};

using namespace adas;

// events == true: everything on one stream with section events (per-stage timing).
// events == false: the lane branch (net + decode) runs on st_lane, forked/joined with events, so the
// latency-bound detector layers and the MFMA-bound lane layers share the chip (independent work:
// demo.py:261-281 runs them back to back only because the reference is single-threaded Python).
static int record_step(adas_pipeline* p, const float* d_det, const float* d_lane, bool events) {
    const int NS = p->d.n_streams;                                   // streams (tracker instances)
    const int B = p->d.micro_batch > 1 ? p->d.micro_batch : 1;       // consecutive frames of each stream in this step
    const int S = NS * B;                                            // frames through pre-processing, nets, decode and NMS
    hipStream_t st = p->st;
    const bool fork = !events && p->d.detector && p->d.lane && !(p->d.use_graph & 2);
    hipStream_t sl = fork ? p->st_lane : st;
    int rc;
    if (events) ADAS_HIP_TRY(hipEventRecord(p->ev[0], st));
    if (fork) {
        ADAS_HIP_TRY(hipEventRecord(p->ev_fork, st));
        ADAS_HIP_TRY(hipStreamWaitEvent(sl, p->ev_fork, 0));
    }
    if (p->fsrc.frames) {  // pre-processing inside the step: each branch converts the shared u8 frames for its own net
        if (p->d.detector) {
            int64_t is[4];
            adas_engine_input_shape(p->d.detector, is);
            rc = p->packed ? adas_preprocess_yolo_packed_prec(p->fsrc.frames, S, p->fsrc.h, p->fsrc.w, (uint16_t*)p->det_in, (int)is[2], (int)is[3], 1,
                                                              p->d.detector->prec, st)
                           : adas_preprocess_yolo(p->fsrc.frames, S, p->fsrc.h, p->fsrc.w, p->det_in, (int)is[2], (int)is[3], 1, st);
            if (rc) return rc;
        }
        if (p->d.lane) {
            int64_t is[4];
            adas_engine_input_shape(p->d.lane, is);
            rc = p->packed ? adas_preprocess_ufld_packed_prec(p->fsrc.frames, S, p->fsrc.h, p->fsrc.w, (uint16_t*)p->lane_in, (int)is[2], (int)is[3], p->fsrc.crop,
                                                              p->d.lane->prec, sl)
                           : adas_preprocess_ufld(p->fsrc.frames, S, p->fsrc.h, p->fsrc.w, p->lane_in, (int)is[2], (int)is[3], p->fsrc.crop, sl);
            if (rc) return rc;
        }
    }
    const bool packed_now = p->fsrc.frames && p->packed;
    if (p->d.detector) {
        // fused v8 Detect: per-anchor (best probability, class) come straight out of its registers into the post-processing's scan arrays;
        // the head's class rows are not written and the scan launch goes away (ADAS_NO_DETECT_SINK=1: the full head + scan)
        float* sc_conf = nullptr;
        int32_t* sc_cls = nullptr;
        if (p->sink) {
            rc = adas_yolo_post_scan_views(p->d.post, &sc_conf, &sc_cls);
            if (rc) return rc;
            rc = adas_engine_set_detect_sink(p->d.detector, sc_conf, sc_cls);
            if (rc) return rc;
        }
        rc = packed_now ? adas_engine_infer_device_packed(p->d.detector, (const uint16_t*)d_det, S, st) : adas_engine_infer_device(p->d.detector, d_det, S, st);
        if (p->sink) (void)adas_engine_set_detect_sink(p->d.detector, nullptr, nullptr);   // launches are enqueued (or captured) with the sink baked in
        if (rc) return rc;
        if (events) ADAS_HIP_TRY(hipEventRecord(p->ev[1], st));
        rc = p->sink ? adas_yolo_post_run_prescanned(p->d.post, adas_engine_output_device(p->d.detector, 0), S, st)
                     : adas_yolo_post_run(p->d.post, adas_engine_output_device(p->d.detector, 0), S, st);
        if (rc) return rc;
    } else if (events) ADAS_HIP_TRY(hipEventRecord(p->ev[1], st));
    if (events) ADAS_HIP_TRY(hipEventRecord(p->ev[2], st));
    if (p->d.lane) {
        rc = packed_now ? adas_engine_infer_device_packed(p->d.lane, (const uint16_t*)d_lane, S, sl) : adas_engine_infer_device(p->d.lane, d_lane, S, sl);
        if (rc) return rc;
        if (events) ADAS_HIP_TRY(hipEventRecord(p->ev[3], st));
        const adas_engine* le = p->d.lane;
        size_t stride = (size_t)le->bufs[le->outs[0].buf].h * le->bufs[le->outs[0].buf].w * le->bufs[le->outs[0].buf].c;
        if (adas_ufld_decode_kind(p->d.decode) == 1)  // UFLD v1: one (G+1, K, 4) tensor per frame
            rc = adas_ufld1_decode_run(p->d.decode, adas_engine_output_device(le, 0), stride, S, sl);
        else
            rc = adas_ufld_decode_run(p->d.decode, adas_engine_output_device(le, 0), adas_engine_output_device(le, 1),
                                      adas_engine_output_device(le, 2), adas_engine_output_device(le, 3), stride, stride, stride, stride, S, sl);
        if (rc) return rc;
        if (p->bird) {   // this step's trapezoids first: the geometry and the image warp read frame f's matrices from the handle's tables
            const double *d_M, *d_M_warp;
            rc = adas_birdview_device_views(p->bird, &d_M, &d_M_warp);
            if (rc) return rc;
            rc = adas_birdview_run(p->bird, p->d.decode, NS, B, sl);
            if (rc) return rc;
            rc = adas_lane_geometry_run_matrices(p->d.geometry, p->d.decode, -1, S, d_M, sl);
            if (rc) return rc;
            if (p->bird_warp) {
                ADAS_REQUIRE(p->fsrc.frames, ADAS_ERR_INVALID, "the bird-view image needs camera frames: use adas_pipeline_step_frames");
                rc = adas_warp_run_device_matrices(p->bird_warp, p->fsrc.frames, nullptr, d_M_warp, S, sl);
                if (rc) return rc;
            }
        } else if (p->d.geometry) {
            rc = adas_lane_geometry_run(p->d.geometry, p->d.decode, -1, S, sl);
            if (rc) return rc;
        }
    } else if (events) ADAS_HIP_TRY(hipEventRecord(p->ev[3], st));
    if (events) ADAS_HIP_TRY(hipEventRecord(p->ev[4], st));
    if (p->d.tracker && p->d.detector) {
        const double *xy, *sc;
        const int32_t *cl, *cn;
        rc = adas_yolo_post_device_views(p->d.post, &xy, &sc, &cl, &cn);
        if (rc) return rc;
        int cap = 0;
        rc = adas_yolo_post_capacity(p->d.post, &cap);
        if (rc) return rc;
        // frame b of stream s sits at frame index b * NS + s: one launch, every stream's workgroup runs its B updates in temporal order
        rc = B > 1 ? adas_bytetrack_update_device_frames(p->d.tracker, xy, sc, cl, cn, cap, 4, 2, NS, B, st)
                   : adas_bytetrack_update_device(p->d.tracker, xy, sc, cl, cn, cap, 4, 2, NS, st);
        if (rc) return rc;
    }
    if (fork) {
        ADAS_HIP_TRY(hipEventRecord(p->ev_join, sl));
        ADAS_HIP_TRY(hipStreamWaitEvent(st, p->ev_join, 0));
    }
    if (p->analysis) {   // reads both branches' results; its request words meet the NEXT step's adas_birdview_run, ordered through that step's fork
        rc = adas_analysis_run(p->analysis, p->d.post, p->d.geometry, p->bird, NS, B, st);
        if (rc) return rc;
    }
    if (p->overlay) {   // behind the join: the lane branch's points, polygon and warped bird view, and this frame's analysis row, are all there
        ADAS_REQUIRE(p->fsrc.frames, ADAS_ERR_INVALID, "the overlay needs camera frames: use adas_pipeline_step_frames");
        int stages = p->overlay_stages;
        if (stages < 0)
            stages = ADAS_OVERLAY_LANES | ADAS_OVERLAY_AREA | (p->analysis ? ADAS_OVERLAY_DISTANCE : 0) | (p->bird_warp ? ADAS_OVERLAY_BIRD : 0);
        ADAS_REQUIRE(!(stages & ADAS_OVERLAY_DISTANCE) || p->analysis, ADAS_ERR_INVALID, "the overlay's distance stage needs an attached analysis handle");
        ADAS_REQUIRE(!(stages & ADAS_OVERLAY_BIRD) || p->bird_warp, ADAS_ERR_INVALID, "the overlay's bird stage needs an attached bird view with its warp");
        ADAS_REQUIRE(!p->overlay_readouts || p->bird_warp, ADAS_ERR_INVALID, "the overlay's readouts stage needs an attached bird view with its warp");
        stages |= p->overlay_readouts;
        const uint8_t* bird_img = nullptr;
        if (stages & (ADAS_OVERLAY_BIRD | ADAS_OVERLAY_READOUTS)) {
            int oh = 0, ow = 0, obh = 0, obw = 0, ob = 0, wh = 0, ww = 0;
            (void)adas::overlay_geometry(p->overlay, &oh, &ow, &obh, &obw, &ob);
            adas::warp_dst_geometry(p->bird_warp, &wh, &ww);
            ADAS_REQUIRE(obh == wh && obw == ww, ADAS_ERR_INVALID, "the overlay handle was created for a %dx%d bird view, the attached warp writes %dx%d", obh, obw,
                         wh, ww);
            rc = adas_warp_device_view(p->bird_warp, &bird_img);
            if (rc) return rc;
        }
        // the object layer draws this step's survivors and the tracker after this step's update; trajectories under the conditions of tracks
        ADAS_REQUIRE(!(stages & ADAS_OVERLAY_DETECTIONS) || (p->d.detector && p->d.post), ADAS_ERR_INVALID,
                     "the overlay's detections stage needs a detector with its post handle");
        ADAS_REQUIRE(!(stages & ADAS_OVERLAY_TRACKS) || (p->d.tracker && p->d.detector), ADAS_ERR_INVALID,
                     "the overlay's tracks stage needs a tracker (and the detector that feeds it)");
        ADAS_REQUIRE(!(stages & ADAS_OVERLAY_TRAJECTORIES) || (p->d.tracker && p->d.detector), ADAS_ERR_INVALID,
                     "the overlay's trajectories stage needs a tracker (and the detector that feeds it)");
        ADAS_REQUIRE(!(stages & (ADAS_OVERLAY_TRACKS | ADAS_OVERLAY_TRAJECTORIES)) || B <= 1, ADAS_ERR_INVALID,
                     "the overlay's %s stage needs micro_batch <= 1 (got %d): the tracker's live table holds only the last frame of a step",
                     (stages & ADAS_OVERLAY_TRACKS) ? "tracks" : "trajectories", B);
        rc = adas::overlay_run_handles("adas_pipeline_step (overlay)", 63 | ADAS_OVERLAY_TRAJECTORIES | ADAS_OVERLAY_READOUTS, p->overlay,
                                       {p->fsrc.frames, nullptr, p->d.decode, p->d.geometry, p->analysis, p->d.post, p->d.tracker,
                                        const_cast<uint8_t*>(bird_img), stages, NS, B, st});
        if (rc) return rc;
        const int text = p->overlay_text, text_scene = ADAS_TEXT_DETECTIONS | ADAS_TEXT_TRACKS | ADAS_TEXT_TRACK_IDS | ADAS_TEXT_DISTANCE;
        if (text) {   // one layout of every kind; the scene's text is painted now, over the stages and under the panels
            ADAS_REQUIRE(!(text & (ADAS_TEXT_TRACKS | ADAS_TEXT_TRACK_IDS)) || B <= 1, ADAS_ERR_INVALID,
                         "the overlay's %s text needs micro_batch <= 1 (got %d): the tracker's live table holds only the last frame of a step",
                         (text & ADAS_TEXT_TRACKS) ? "tracks" : "track_ids", B);
            rc = adas::overlay_run_text("adas_pipeline_step (overlay text)", p->overlay, nullptr, p->d.detector ? p->d.post : nullptr,
                                        p->d.detector ? p->d.tracker : nullptr, p->analysis, text, text_scene, NS, B, st);
            if (rc) return rc;
        }
        if (p->overlay_panels) {   // directly behind the overlay's run, in place on the frames it just wrote
            const int panels = p->overlay_panels;
            ADAS_REQUIRE(!(panels & (ADAS_PANEL_SIGNS | ADAS_PANEL_COLLISION)) || p->analysis, ADAS_ERR_INVALID,
                         "the overlay's %s panel needs an attached analysis handle", (panels & ADAS_PANEL_SIGNS) ? "signs" : "collision");
            ADAS_REQUIRE(!(panels & ADAS_PANEL_BIRD) || p->bird_warp, ADAS_ERR_INVALID, "the overlay's bird panel needs an attached bird view with its warp");
            if ((panels & ADAS_PANEL_BIRD) && !bird_img) {   // the bird stage is off: the panel shows the warped image without discs
                rc = adas_warp_device_view(p->bird_warp, &bird_img);
                if (rc) return rc;
            }
            rc = adas::overlay_run_panels("adas_pipeline_step (overlay panels)", p->overlay, nullptr, p->analysis, bird_img, panels, NS, B, st);
            if (rc) return rc;
        }
        if (text & ~text_scene) {   // the panel strings and the caller's lines lie over the panels
            rc = adas::overlay_draw_text("adas_pipeline_step (overlay text)", p->overlay, text & ~text_scene, S, st);
            if (rc) return rc;
        }
    }
    if (p->scale) {   // the finished frames as tiles of canvases: behind everything that writes them, read once
        ADAS_REQUIRE(p->fsrc.frames, ADAS_ERR_INVALID, "the scaling stage needs camera frames: use adas_pipeline_step_frames");
        const uint8_t* src = p->fsrc.frames;
        if (p->scale_source == ADAS_SCALE_SRC_OVERLAY) {
            ADAS_REQUIRE(p->overlay, ADAS_ERR_INVALID, "the scaling stage's overlay source needs an attached overlay handle");
            rc = adas_overlay_device_view(p->overlay, &src);
            if (rc) return rc;
        }
        int sw = 0, sh = 0, cw = 0, ch = 0, tiles = 0, sb = 0, border = 0;
        adas::scale_geometry_of(p->scale, &sw, &sh, &cw, &ch, &tiles, &sb, &border);
        const int* col = nullptr;
        int stride = 0;
        if (border > 0) {   // the tiles wear their frames' collision state
            ADAS_REQUIRE(p->analysis, ADAS_ERR_INVALID, "the scaling stage's border needs an attached analysis handle");
            const int *fr, *pts;
            int maxp = 0;
            adas::analysis_frame_views(p->analysis, &fr, &stride, &pts, &maxp);
            col = fr + offsetof(adas_analysis_frame, collision_msg) / 4;
        }
        rc = adas_scale_run(p->scale, src, S, col, (int64_t)stride * 4, nullptr, st);
        if (rc) return rc;
        const uint8_t* canvases = nullptr;
        rc = adas_scale_device_view(p->scale, &canvases);
        if (rc) return rc;
        const int n = (S + tiles - 1) / tiles;
        if (p->scale_jpeg) {
            rc = adas_jpeg_run(p->scale_jpeg, canvases, n, st);
            if (rc) return rc;
        }
        if (p->scale_yuvout) {
            rc = adas_yuvout_run(p->scale_yuvout, canvases, n, nullptr, st);
            if (rc) return rc;
        }
    }
    if (p->jpeg) {   // the finished frames leave as compressed streams: behind everything that writes them
        ADAS_REQUIRE(p->fsrc.frames, ADAS_ERR_INVALID, "the JPEG stage needs camera frames: use adas_pipeline_step_frames");
        const uint8_t* src = p->fsrc.frames;
        if (p->jpeg_source == ADAS_JPEG_SRC_OVERLAY) {
            ADAS_REQUIRE(p->overlay, ADAS_ERR_INVALID, "the JPEG stage's overlay source needs an attached overlay handle");
            rc = adas_overlay_device_view(p->overlay, &src);
            if (rc) return rc;
        }
        rc = adas_jpeg_run(p->jpeg, src, S, st);
        if (rc) return rc;
    }
    if (p->yuvout) {   // and as raw video: reads the same finished frames, writes its own buffer
        ADAS_REQUIRE(p->fsrc.frames, ADAS_ERR_INVALID, "the YUV output stage needs camera frames: use adas_pipeline_step_frames");
        const uint8_t* src = p->fsrc.frames;
        if (p->yuvout_source == ADAS_YUVOUT_SRC_OVERLAY) {
            ADAS_REQUIRE(p->overlay, ADAS_ERR_INVALID, "the YUV output stage's overlay source needs an attached overlay handle");
            rc = adas_overlay_device_view(p->overlay, &src);
            if (rc) return rc;
        }
        rc = adas_yuvout_run(p->yuvout, src, S, nullptr, st);
        if (rc) return rc;
    }
    if (events) ADAS_HIP_TRY(hipEventRecord(p->ev[5], st));
    return ADAS_OK;
}

static void drop_graphs(adas_pipeline* p) {
    for (auto& g : p->graphs) {
        if (g.exec) (void)hipGraphExecDestroy(g.exec);
        if (g.graph) (void)hipGraphDestroy(g.graph);
    }
    p->graphs.clear();
    p->last_graph = nullptr;
}

extern "C" {

int adas_pipeline_create(const adas_pipeline_desc* d, adas_pipeline** out) {
    ADAS_REQUIRE(d && out && d->n_streams > 0, ADAS_ERR_INVALID, "adas_pipeline_create: bad argument");
    ADAS_REQUIRE(d->detector || d->lane, ADAS_ERR_INVALID, "pipeline needs a detector and/or a lane engine");
    ADAS_REQUIRE(!d->detector || d->post, ADAS_ERR_INVALID, "detector engine needs a yolo_post handle");
    ADAS_REQUIRE(!d->lane || d->decode, ADAS_ERR_INVALID, "lane engine needs a ufld_decode handle");
    const int lane_outs = d->lane ? (adas_ufld_decode_kind(d->decode) == 1 ? 1 : 4) : 0;  // ultrafastLaneDetector.py:73-75 | V2:93-94
    ADAS_REQUIRE(!d->lane || adas_engine_num_outputs(d->lane) == lane_outs, ADAS_ERR_INVALID,
                 "Output dims is error, please check model. load %d channels not match %d.", d->lane ? adas_engine_num_outputs(d->lane) : 0, lane_outs);
    if (d->detector) {  // the post kernel indexes the head by ITS (layout, A, nc): a mismatch would read past the engine's buffer
        int32_t layout = 0, A = 0, nc = 0;
        int rc0 = adas_yolo_post_head_shape(d->post, &layout, &A, &nc);
        if (rc0) return rc0;
        int64_t od[4] = {0, 0, 0, 0};
        int nd = 0;
        ADAS_REQUIRE(adas_engine_num_outputs(d->detector) >= 1 && adas_engine_output_shape(d->detector, 0, od, &nd) == ADAS_OK && nd == 3,
                     ADAS_ERR_INVALID, "detector engine has no (1, C, A) / (1, A, C) head output");
        const int64_t want1 = layout == ADAS_HEAD_V8 ? 4 + nc : A, want2 = layout == ADAS_HEAD_V8 ? A : 5 + nc;
        ADAS_REQUIRE(od[1] == want1 && od[2] == want2, ADAS_ERR_INVALID,
                     "detector head is (1,%lld,%lld) but the post-processor was created for (1,%lld,%lld) [layout %d, %d anchors, %d classes]",
                     (long long)od[1], (long long)od[2], (long long)want1, (long long)want2, layout, A, nc);
    }
    if (d->lane) {
        int64_t want[4][4];
        const int n = adas_ufld_decode_expected_outputs(d->decode, want);
        for (int i = 0; i < n; ++i) {
            int64_t od[4] = {0, 0, 0, 0};
            int nd = 0;
            ADAS_REQUIRE(adas_engine_output_shape(d->lane, i, od, &nd) == ADAS_OK && nd == 4 && od[1] == want[i][1] && od[2] == want[i][2] && od[3] == want[i][3],
                         ADAS_ERR_INVALID, "lane output %d is (1,%lld,%lld,%lld) but the decoder was created for (1,%lld,%lld,%lld)", i, (long long)od[1],
                         (long long)od[2], (long long)od[3], (long long)want[i][1], (long long)want[i][2], (long long)want[i][3]);
        }
    }
    const int frames_per_step = d->n_streams * (d->micro_batch > 1 ? d->micro_batch : 1);
    ADAS_REQUIRE(d->micro_batch >= 0 && d->micro_batch <= 64, ADAS_ERR_INVALID, "micro_batch must be in [0, 64]");
    ADAS_REQUIRE(!d->detector || frames_per_step <= d->detector->max_batch, ADAS_ERR_INVALID, "n_streams x micro_batch exceeds detector max_batch");
    ADAS_REQUIRE(!d->lane || frames_per_step <= d->lane->max_batch, ADAS_ERR_INVALID, "n_streams x micro_batch exceeds lane max_batch");
    // the post-processing handles index per-frame arenas: too small a handle must fail here, not inside the first (captured) step
    ADAS_REQUIRE(!d->post || frames_per_step <= adas::handle_max_batch(d->post), ADAS_ERR_INVALID,
                 "n_streams x micro_batch = %d exceeds the yolo_post handle's max_batch %d", frames_per_step, adas::handle_max_batch(d->post));
    ADAS_REQUIRE(!d->decode || frames_per_step <= adas::handle_max_batch(d->decode), ADAS_ERR_INVALID,
                 "n_streams x micro_batch = %d exceeds the ufld_decode handle's max_batch %d", frames_per_step, adas::handle_max_batch(d->decode));
    ADAS_REQUIRE(!d->geometry || frames_per_step <= adas::handle_max_batch(d->geometry), ADAS_ERR_INVALID,
                 "n_streams x micro_batch = %d exceeds the lane_geometry handle's max_batch %d", frames_per_step, adas::handle_max_batch(d->geometry));
    adas_pipeline* p = new adas_pipeline();
    p->d = *d;
    if (hipStreamCreateWithFlags(&p->st, hipStreamNonBlocking) != hipSuccess) {
        delete p;
        return hip_fail(hipGetLastError(), "hipStreamCreate", __FILE__, __LINE__);
    }
    if (hipStreamCreateWithFlags(&p->st_lane, hipStreamNonBlocking) != hipSuccess) {
        adas_pipeline_destroy(p);
        return hip_fail(hipGetLastError(), "hipStreamCreate", __FILE__, __LINE__);
    }
    for (auto& e : p->ev)
        if (hipEventCreate(&e) != hipSuccess) {
            adas_pipeline_destroy(p);
            return hip_fail(hipGetLastError(), "hipEventCreate", __FILE__, __LINE__);
        }
    if (hipEventCreateWithFlags(&p->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&p->ev_join, hipEventDisableTiming) != hipSuccess) {
        adas_pipeline_destroy(p);
        return hip_fail(hipGetLastError(), "hipEventCreate", __FILE__, __LINE__);
    }
    if (d->tracker && d->detector && d->micro_batch > 1) {   // every frame's tracker message stays fetchable (adas_bytetrack_fetch_frame)
        int rc = adas_bytetrack_reserve_frames(d->tracker, d->micro_batch, d->n_streams);
        if (rc) {
            adas_pipeline_destroy(p);
            return rc;
        }
    }
    if (d->detector && d->post) {
        // only when the post-processing was created for exactly the head the engine's fused Detect describes (its scan arrays hold
        // [max_batch][num_anchors] entries of that layout)
        int32_t layout = -1, pa = 0, pn = 0, el = -2, ea = 0, en = 0;
        const char* env = getenv("ADAS_NO_DETECT_SINK");
        (void)adas_yolo_post_head_shape(d->post, &layout, &pa, &pn);
        p->sink = adas_engine_detect_sink_supported(d->detector) && adas_engine_detect_sink_shape(d->detector, &el, &ea, &en) == ADAS_OK &&
                  el == layout && ea == pa && en == pn && !(env && env[0] == '1');
    }
    *out = p;
    return ADAS_OK;
}
int adas_pipeline_detect_sink(const adas_pipeline* p) { return p && p->sink ? 1 : 0; }

int adas_pipeline_attach_birdview(adas_pipeline* p, adas_birdview* bird, adas_warp* warp) {
    ADAS_REQUIRE(p && bird, ADAS_ERR_INVALID, "adas_pipeline_attach_birdview: bad argument");
    ADAS_REQUIRE(p->d.lane && p->d.decode && p->d.geometry, ADAS_ERR_INVALID,
                 "adas_pipeline_attach_birdview: the pipeline needs a lane engine, a decode handle and a geometry handle");
    const int frames = p->d.n_streams * (p->d.micro_batch > 1 ? p->d.micro_batch : 1);
    int bs = 0, bf = 0;
    (void)adas::birdview_capacity(bird, &bs, &bf);
    ADAS_REQUIRE(bs >= p->d.n_streams && bf >= frames, ADAS_ERR_INVALID,
                 "adas_pipeline_attach_birdview: the handle holds %d streams / %d frames, a step has %d streams / %d frames", bs, bf, p->d.n_streams, frames);
    if (warp) {
        int sh = 0, sw = 0, wb = 0;
        (void)adas::warp_geometry(warp, &sh, &sw, &wb);
        ADAS_REQUIRE(wb >= frames, ADAS_ERR_INVALID, "adas_pipeline_attach_birdview: the warp handle holds %d frames, a step has %d", wb, frames);
        const uint8_t* own = nullptr;   // its buffer exists before the first (captured) step
        int rc = adas_warp_device_view(warp, &own);
        if (rc) return rc;
    }
    ADAS_REQUIRE(!p->analysis || p->d.micro_batch <= 1, ADAS_ERR_INVALID,
                 "adas_pipeline_attach_birdview: an analysis handle is attached and micro_batch is %d: a frame's request cannot reach the next frame "
                 "inside one step", p->d.micro_batch);
    ADAS_HIP_TRY(hipStreamSynchronize(p->st));
    drop_graphs(p);
    p->bird = bird;
    p->bird_warp = warp;
    if (p->analysis) return adas::analysis_bind_birdview(p->analysis, bird, p->d.n_streams, p->st);
    return ADAS_OK;
}

int adas_pipeline_attach_analysis(adas_pipeline* p, adas_analysis* analysis) {
    ADAS_REQUIRE(p && analysis, ADAS_ERR_INVALID, "adas_pipeline_attach_analysis: bad argument");
    ADAS_REQUIRE(p->d.detector && p->d.post && p->d.lane && p->d.decode && p->d.geometry, ADAS_ERR_INVALID,
                 "adas_pipeline_attach_analysis: the pipeline needs a detector with its post handle and a lane engine with decode and geometry handles");
    ADAS_REQUIRE(!p->bird || p->d.micro_batch <= 1, ADAS_ERR_INVALID,
                 "adas_pipeline_attach_analysis: a bird-view handle is attached and micro_batch is %d: a frame's request cannot reach the next frame "
                 "inside one step", p->d.micro_batch);
    const int frames = p->d.n_streams * (p->d.micro_batch > 1 ? p->d.micro_batch : 1);
    int as = 0, af = 0;
    (void)adas::analysis_capacity(analysis, &as, &af);
    ADAS_REQUIRE(as >= p->d.n_streams && af >= frames, ADAS_ERR_INVALID,
                 "adas_pipeline_attach_analysis: the handle holds %d streams / %d frames, a step has %d streams / %d frames", as, af, p->d.n_streams, frames);
    ADAS_HIP_TRY(hipStreamSynchronize(p->st));
    drop_graphs(p);
    p->analysis = analysis;
    return adas::analysis_bind_birdview(analysis, p->bird, p->d.n_streams, p->st);
}

int adas_pipeline_attach_overlay(adas_pipeline* p, adas_overlay* overlay) {
    ADAS_REQUIRE(p && overlay, ADAS_ERR_INVALID, "adas_pipeline_attach_overlay: bad argument");
    ADAS_REQUIRE(p->d.lane && p->d.decode && p->d.geometry, ADAS_ERR_INVALID,
                 "adas_pipeline_attach_overlay: the pipeline needs a lane engine, a decode handle and a geometry handle");
    ADAS_REQUIRE(adas::decode_num_lanes(p->d.decode) == 4, ADAS_ERR_INVALID,
                 "adas_pipeline_attach_overlay: the decoder has num_lanes = %d (CurveLanes); the overlay draws the reference's four lane colours, num_lanes "
                 "must be 4", adas::decode_num_lanes(p->d.decode));
    const int frames = p->d.n_streams * (p->d.micro_batch > 1 ? p->d.micro_batch : 1);
    int oh = 0, ow = 0, obh = 0, obw = 0, ob = 0;
    (void)adas::overlay_geometry(overlay, &oh, &ow, &obh, &obw, &ob);
    ADAS_REQUIRE(ob >= frames, ADAS_ERR_INVALID, "adas_pipeline_attach_overlay: the overlay handle holds %d frames, a step has %d", ob, frames);
    if (p->bird_warp && obh > 0) {
        int wh = 0, ww = 0;
        adas::warp_dst_geometry(p->bird_warp, &wh, &ww);
        ADAS_REQUIRE(obh == wh && obw == ww, ADAS_ERR_INVALID,
                     "adas_pipeline_attach_overlay: the overlay handle was created for a %dx%d bird view, the attached warp writes %dx%d", obh, obw, wh, ww);
    }
    const uint8_t* own = nullptr;   // its buffer exists before the first (captured) step
    int rc = adas_overlay_device_view(overlay, &own);
    if (rc) return rc;
    ADAS_HIP_TRY(hipStreamSynchronize(p->st));
    drop_graphs(p);
    p->overlay = overlay;
    p->overlay_stages = -1;
    p->overlay_panels = 0;
    p->overlay_text = 0;
    p->overlay_readouts = 0;
    return ADAS_OK;
}

int adas_pipeline_set_overlay_stages(adas_pipeline* p, int stages) {
    ADAS_REQUIRE(p && p->overlay, ADAS_ERR_INVALID, "adas_pipeline_set_overlay_stages: no overlay handle attached");
    ADAS_REQUIRE(stages >= 0 && !(stages & ~(63 | ADAS_OVERLAY_TRAJECTORIES)), ADAS_ERR_INVALID, "adas_pipeline_set_overlay_stages: unknown stage bits 0x%x",
                 stages);
    ADAS_HIP_TRY(hipStreamSynchronize(p->st));
    drop_graphs(p);
    int det_cap = 0, trk_cap = 0;
    if ((stages & (ADAS_OVERLAY_TRACKS | ADAS_OVERLAY_TRAJECTORIES)) && p->d.tracker) {
        int ts = 0;
        const unsigned char *hdr, *out;
        size_t sb = 0;
        adas::tracker_live_views(p->d.tracker, &hdr, &out, &sb, &ts, &trk_cap);
    }
    if (stages & (ADAS_OVERLAY_DETECTIONS | ADAS_OVERLAY_TRACKS)) {   // the boxes' records are allocated now: a captured step cannot
        const int *a, *b, *c;
        if ((stages & ADAS_OVERLAY_DETECTIONS) && p->d.post) adas::post_survivor_views(p->d.post, &a, &b, &c, &det_cap);
        int rc = adas::overlay_reserve_objects(p->overlay, det_cap, (stages & ADAS_OVERLAY_TRACKS) ? trk_cap : 0);
        if (rc) return rc;
    }
    if ((stages & ADAS_OVERLAY_TRAJECTORIES) && p->d.tracker) {   // so are the tracks' primitives and their plane
        int rc = adas::overlay_reserve_trajectories(p->overlay, trk_cap);
        if (rc) return rc;
    }
    p->overlay_stages = stages;
    return ADAS_OK;
}

int adas_pipeline_set_overlay_panels(adas_pipeline* p, int panels) {
    ADAS_REQUIRE(p && p->overlay, ADAS_ERR_INVALID, "adas_pipeline_set_overlay_panels: no overlay handle attached");
    ADAS_REQUIRE(panels >= 0 && !(panels & ~(ADAS_PANEL_BIRD | ADAS_PANEL_SIGNS | ADAS_PANEL_COLLISION)), ADAS_ERR_INVALID,
                 "adas_pipeline_set_overlay_panels: unknown panel bits 0x%x", panels);
    ADAS_REQUIRE(!panels || adas::overlay_panels_ready(p->overlay), ADAS_ERR_INVALID,
                 "adas_pipeline_set_overlay_panels: no panels set on the attached overlay handle (call adas_overlay_set_panels first)");
    ADAS_HIP_TRY(hipStreamSynchronize(p->st));
    drop_graphs(p);
    p->overlay_panels = panels;
    return ADAS_OK;
}

int adas_pipeline_set_overlay_text(adas_pipeline* p, int mask) {
    ADAS_REQUIRE(p && p->overlay, ADAS_ERR_INVALID, "adas_pipeline_set_overlay_text: no overlay handle attached");
    ADAS_REQUIRE(mask >= 0 && !(mask & ~63), ADAS_ERR_INVALID, "adas_pipeline_set_overlay_text: unknown text bits 0x%x", mask);
    ADAS_REQUIRE(!mask || adas::overlay_text_ready(p->overlay), ADAS_ERR_INVALID,
                 "adas_pipeline_set_overlay_text: no font set on the attached overlay handle (call adas_overlay_set_font first)");
    ADAS_HIP_TRY(hipStreamSynchronize(p->st));
    drop_graphs(p);
    p->overlay_text = mask;
    return ADAS_OK;
}

int adas_pipeline_set_overlay_readouts(adas_pipeline* p, int on) {
    ADAS_REQUIRE(p && p->overlay, ADAS_ERR_INVALID, "adas_pipeline_set_overlay_readouts: no overlay handle attached");
    if (on) {   // the records are allocated now (a captured step cannot), and the font must be there
        int rc = adas::overlay_readout_reserve(p->overlay);
        if (!rc) rc = adas::overlay_readout_check("adas_pipeline_set_overlay_readouts", p->overlay);
        if (rc) return rc;
    }
    ADAS_HIP_TRY(hipStreamSynchronize(p->st));
    drop_graphs(p);
    p->overlay_readouts = on ? ADAS_OVERLAY_READOUTS : 0;
    return ADAS_OK;
}

int adas_pipeline_attach_jpeg(adas_pipeline* p, adas_jpeg* jpeg, int source) {
    ADAS_REQUIRE(p, ADAS_ERR_INVALID, "adas_pipeline_attach_jpeg: null pipeline");
    if (jpeg) {
        ADAS_REQUIRE(source == ADAS_JPEG_SRC_OVERLAY || source == ADAS_JPEG_SRC_FRAMES, ADAS_ERR_INVALID, "adas_pipeline_attach_jpeg: unknown source %d",
                     source);
        ADAS_REQUIRE(source != ADAS_JPEG_SRC_OVERLAY || p->overlay, ADAS_ERR_INVALID,
                     "adas_pipeline_attach_jpeg: the overlay source needs an attached overlay handle (adas_pipeline_attach_overlay first)");
        const int frames = p->d.n_streams * (p->d.micro_batch > 1 ? p->d.micro_batch : 1);
        int jw = 0, jh = 0, jb = 0;
        adas::jpeg_geometry_of(jpeg, &jw, &jh, &jb);
        ADAS_REQUIRE(jb >= frames, ADAS_ERR_INVALID, "adas_pipeline_attach_jpeg: the JPEG handle holds %d frames, a step has %d", jb, frames);
        if (source == ADAS_JPEG_SRC_OVERLAY) {
            int oh = 0, ow = 0, obh = 0, obw = 0, ob = 0;
            (void)adas::overlay_geometry(p->overlay, &oh, &ow, &obh, &obw, &ob);
            ADAS_REQUIRE(oh == jh && ow == jw, ADAS_ERR_INVALID,
                         "adas_pipeline_attach_jpeg: the JPEG handle was created for %dx%d frames, the attached overlay draws %dx%d", jw, jh, ow, oh);
        }
    }
    ADAS_HIP_TRY(hipStreamSynchronize(p->st));
    drop_graphs(p);
    p->jpeg = jpeg;
    p->jpeg_source = source;
    return ADAS_OK;
}

int adas_pipeline_attach_yuvout(adas_pipeline* p, adas_yuvout* yuvout, int source) {
    ADAS_REQUIRE(p, ADAS_ERR_INVALID, "adas_pipeline_attach_yuvout: null pipeline");
    if (yuvout) {
        ADAS_REQUIRE(source == ADAS_YUVOUT_SRC_OVERLAY || source == ADAS_YUVOUT_SRC_FRAMES, ADAS_ERR_INVALID,
                     "adas_pipeline_attach_yuvout: unknown source %d", source);
        ADAS_REQUIRE(source != ADAS_YUVOUT_SRC_OVERLAY || p->overlay, ADAS_ERR_INVALID,
                     "adas_pipeline_attach_yuvout: the overlay source needs an attached overlay handle (adas_pipeline_attach_overlay first)");
        const int frames = p->d.n_streams * (p->d.micro_batch > 1 ? p->d.micro_batch : 1);
        int yw = 0, yh = 0, yb = 0;
        adas::yuvout_geometry_of(yuvout, &yw, &yh, &yb);
        ADAS_REQUIRE(yb >= frames, ADAS_ERR_INVALID, "adas_pipeline_attach_yuvout: the YUV output handle holds %d frames, a step has %d", yb, frames);
        if (source == ADAS_YUVOUT_SRC_OVERLAY) {
            int oh = 0, ow = 0, obh = 0, obw = 0, ob = 0;
            (void)adas::overlay_geometry(p->overlay, &oh, &ow, &obh, &obw, &ob);
            ADAS_REQUIRE(oh == yh && ow == yw, ADAS_ERR_INVALID,
                         "adas_pipeline_attach_yuvout: the YUV output handle was created for %dx%d frames, the attached overlay draws %dx%d", yw, yh, ow,
                         oh);
        }
    }
    ADAS_HIP_TRY(hipStreamSynchronize(p->st));
    drop_graphs(p);
    p->yuvout = yuvout;
    p->yuvout_source = source;
    return ADAS_OK;
}

int adas_pipeline_graph_kernels(adas_pipeline* p, int32_t* n_kernels) {
    ADAS_REQUIRE(p && n_kernels, ADAS_ERR_INVALID, "adas_pipeline_graph_kernels: bad argument");
    ADAS_REQUIRE(p->last_graph, ADAS_ERR_INVALID, "adas_pipeline_graph_kernels: no captured step has been replayed yet");
    size_t n = 0;
    ADAS_HIP_TRY(hipGraphGetNodes(p->last_graph, nullptr, &n));
    std::vector<hipGraphNode_t> nodes(n);
    if (n) ADAS_HIP_TRY(hipGraphGetNodes(p->last_graph, nodes.data(), &n));
    int k = 0;
    for (size_t i = 0; i < n; ++i) {
        hipGraphNodeType t;
        ADAS_HIP_TRY(hipGraphNodeGetType(nodes[i], &t));
        if (t == hipGraphNodeTypeKernel) ++k;
    }
    *n_kernels = k;
    return ADAS_OK;
}

int adas_pipeline_request_transform(adas_pipeline* p, int stream, int mode) {
    ADAS_REQUIRE(p && p->bird, ADAS_ERR_INVALID, "adas_pipeline_request_transform: no bird-view handle attached");
    ADAS_REQUIRE(!p->analysis, ADAS_ERR_INVALID, "adas_pipeline_request_transform: an analysis handle is attached, the device owns the requests");
    ADAS_REQUIRE(stream >= 0 && stream < p->d.n_streams, ADAS_ERR_INVALID, "adas_pipeline_request_transform: stream %d of %d", stream, p->d.n_streams);
    return adas_birdview_request(p->bird, stream, mode, p->st);   // ordered ahead of the next step on the pipeline's stream; no re-capture
}

int adas_pipeline_destroy(adas_pipeline* p) {
    if (!p) return ADAS_OK;
    drop_graphs(p);
    if (p->analysis) (void)adas::analysis_bind_birdview(p->analysis, nullptr, 0, nullptr);   // its reset no longer queues on this pipeline's stream
    if (p->remap) {   // nor do the remap handle's set calls and fetches
        if (p->st) (void)hipStreamSynchronize(p->st);
        adas::remap_forget_stream(p->remap);
    }
    for (auto& e : p->ev)
        if (e) (void)hipEventDestroy(e);
    if (p->ev_fork) (void)hipEventDestroy(p->ev_fork);
    if (p->ev_join) (void)hipEventDestroy(p->ev_join);
    if (p->st_lane) (void)hipStreamDestroy(p->st_lane);
    if (p->st) (void)hipStreamDestroy(p->st);
    if (p->det_in) (void)hipFree(p->det_in);
    if (p->lane_in) (void)hipFree(p->lane_in);
    for (int k = 0; k < 2; ++k) {
        if (p->host_stage[k]) (void)hipFree(p->host_stage[k]);
        if (p->ev_copied[k]) (void)hipEventDestroy(p->ev_copied[k]);
        if (p->ev_consumed[k]) (void)hipEventDestroy(p->ev_consumed[k]);
        if (p->ev_jcopied[k]) (void)hipEventDestroy(p->ev_jcopied[k]);
        if (p->ev_jconsumed[k]) (void)hipEventDestroy(p->ev_jconsumed[k]);
        if (p->yuv_stage[k]) (void)hipFree(p->yuv_stage[k]);
        if (p->ev_ycopied[k]) (void)hipEventDestroy(p->ev_ycopied[k]);
        if (p->ev_yconsumed[k]) (void)hipEventDestroy(p->ev_yconsumed[k]);
    }
    if (p->st_copy) (void)hipStreamDestroy(p->st_copy);
    delete p;
    return ADAS_OK;
}

// Replays the captured step for `key`, capturing it first when no capture of the current configuration exists.
static int replay_step(adas_pipeline* p, const adas_pipeline::GraphKey& key, const float* d_det, const float* d_lane,
                       const adas_pipeline::FrameSrc* fs) {
    const unsigned long long gen = adas::config_generation();
    if (gen != p->graphs_gen) {  // a post / decode / geometry setter ran since the captures were made: their arguments are stale
        ADAS_HIP_TRY(hipStreamSynchronize(p->st));
        drop_graphs(p);
        p->graphs_gen = gen;
    }
    hipGraphExec_t exec = nullptr;
    for (auto& g : p->graphs)
        if (g.key == key) {
            exec = g.exec;
            p->last_graph = g.graph;
        }
    if (!exec) {
        ADAS_REQUIRE(p->graphs.size() < 64, ADAS_ERR_CAPACITY, "more than 64 distinct input buffers: reuse staging buffers with use_graph");
        adas_pipeline::Cached g{key, nullptr, nullptr};
        if (fs) p->fsrc = *fs;
        {   // device tables of the engines' multi-layer launches are built BEFORE the capture (allocations and copies cannot be captured)
            const int frames = p->d.n_streams * (p->d.micro_batch > 1 ? p->d.micro_batch : 1);
            int prc = p->d.detector ? adas::engine_prepare(p->d.detector, frames) : ADAS_OK;
            if (prc == ADAS_OK && p->d.lane) prc = adas::engine_prepare(p->d.lane, frames);
            if (prc != ADAS_OK) return prc;
        }
        ADAS_HIP_TRY(hipStreamBeginCapture(p->st, hipStreamCaptureModeThreadLocal));
        int rc = record_step(p, d_det, d_lane, false);
        hipError_t ce = hipStreamEndCapture(p->st, &g.graph);
        p->fsrc.frames = nullptr;
        if (rc == ADAS_OK && ce != hipSuccess) rc = hip_fail(ce, "hipStreamEndCapture", __FILE__, __LINE__);
        if (rc == ADAS_OK) {
            hipError_t ie = hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0);
            if (ie != hipSuccess) rc = hip_fail(ie, "hipGraphInstantiate", __FILE__, __LINE__);
        }
        if (rc != ADAS_OK) {  // nothing half-built stays behind
            if (g.graph) (void)hipGraphDestroy(g.graph);
            (void)hipGetLastError();
            return rc;
        }
        p->graphs.push_back(g);
        exec = g.exec;
        p->last_graph = g.graph;
    }
    ADAS_HIP_TRY(hipEventRecord(p->ev[0], p->st));
    ADAS_HIP_TRY(hipGraphLaunch(exec, p->st));
    ADAS_HIP_TRY(hipEventRecord(p->ev[5], p->st));
    p->timed = false;
    return ADAS_OK;
}

int adas_pipeline_step(adas_pipeline* p, const float* d_det, const float* d_lane) {
    ADAS_REQUIRE(p, ADAS_ERR_INVALID, "null pipeline");
    ADAS_REQUIRE(!p->d.detector || d_det, ADAS_ERR_INVALID, "detector input missing");
    ADAS_REQUIRE(!p->d.lane || d_lane, ADAS_ERR_INVALID, "lane input missing");
    ADAS_REQUIRE(!p->bird_warp, ADAS_ERR_INVALID, "a bird-view image warp is attached: seam tensors carry no frame to warp, use adas_pipeline_step_frames");
    ADAS_REQUIRE(!p->overlay, ADAS_ERR_INVALID, "an overlay is attached: seam tensors carry no frame to draw on, use adas_pipeline_step_frames");
    ADAS_REQUIRE(!p->jpeg, ADAS_ERR_INVALID, "a JPEG stage is attached: seam tensors carry no frame to encode, use adas_pipeline_step_frames");
    ADAS_REQUIRE(!p->yuvout, ADAS_ERR_INVALID,
                 "a YUV output stage is attached: seam tensors carry no frame to convert, use adas_pipeline_step_frames");
    ADAS_REQUIRE(!p->scale, ADAS_ERR_INVALID, "a scaling stage is attached: seam tensors carry no frame to scale, use adas_pipeline_step_frames");
    if (!(p->d.use_graph & 1)) {
        p->timed = true;
        return record_step(p, d_det, d_lane, true);
    }
    return replay_step(p, adas_pipeline::GraphKey{d_det, d_lane, 0, 0, 0.0}, d_det, d_lane, nullptr);
}

int adas_pipeline_step_frames(adas_pipeline* p, const uint8_t* d_frames_bgr, int src_h, int src_w, double lane_crop_ratio) {
    ADAS_REQUIRE(p && d_frames_bgr && src_h > 0 && src_w > 0, ADAS_ERR_INVALID, "adas_pipeline_step_frames: bad argument");
    ADAS_REQUIRE(!p->d.lane || (lane_crop_ratio > 0.0 && lane_crop_ratio <= 1.0), ADAS_ERR_INVALID, "lane crop ratio must be in (0, 1]");
    if (p->bird_warp) {   // the warp reads the step's frames with its own source geometry
        int sh = 0, sw = 0, wb = 0;
        (void)adas::warp_geometry(p->bird_warp, &sh, &sw, &wb);
        ADAS_REQUIRE(sh == src_h && sw == src_w, ADAS_ERR_INVALID, "the attached warp handle was created for %dx%d source frames, the step has %dx%d", sh, sw,
                     src_h, src_w);
    }
    if (p->overlay) {   // so does the overlay
        int oh = 0, ow = 0, obh = 0, obw = 0, ob = 0;
        (void)adas::overlay_geometry(p->overlay, &oh, &ow, &obh, &obw, &ob);
        ADAS_REQUIRE(oh == src_h && ow == src_w, ADAS_ERR_INVALID, "the attached overlay handle was created for %dx%d frames, the step has %dx%d", oh, ow, src_h,
                     src_w);
    }
    if (p->jpeg) {   // and the JPEG stage
        int jw = 0, jh = 0, jb = 0;
        adas::jpeg_geometry_of(p->jpeg, &jw, &jh, &jb);
        ADAS_REQUIRE(jh == src_h && jw == src_w, ADAS_ERR_INVALID, "the attached JPEG handle was created for %dx%d frames, the step has %dx%d", jw, jh, src_w,
                     src_h);
    }
    if (p->yuvout) {   // and the YUV output stage
        int yw = 0, yh = 0, yb = 0;
        adas::yuvout_geometry_of(p->yuvout, &yw, &yh, &yb);
        ADAS_REQUIRE(yh == src_h && yw == src_w, ADAS_ERR_INVALID, "the attached YUV output handle was created for %dx%d frames, the step has %dx%d", yw, yh,
                     src_w, src_h);
    }
    if (p->scale) {   // and the scaling stage
        int sw = 0, sh = 0, cw = 0, ch = 0, tiles = 0, sb = 0, border = 0;
        adas::scale_geometry_of(p->scale, &sw, &sh, &cw, &ch, &tiles, &sb, &border);
        ADAS_REQUIRE(sh == src_h && sw == src_w, ADAS_ERR_INVALID, "the attached scale handle was created for %dx%d frames, the step has %dx%d", sw, sh, src_w,
                     src_h);
    }
    const size_t S = (size_t)p->d.n_streams * (p->d.micro_batch > 1 ? p->d.micro_batch : 1);
    if (p->remap) {   // outside the captured step, like the decoder and the converter: the step below reads the handle's own frames
        int rsh = 0, rsw = 0, rdh = 0, rdw = 0, rns = 0, rb = 0;
        adas::remap_geometry_of(p->remap, &rsh, &rsw, &rdh, &rdw, &rns, &rb);
        ADAS_REQUIRE(rsh == src_h && rsw == src_w, ADAS_ERR_INVALID, "the attached remap handle was created for %dx%d frames, the step has %dx%d", rsw, rsh,
                     src_w, src_h);
        int rc = adas_remap_run(p->remap, d_frames_bgr, (int)S, nullptr, p->st);
        if (rc) return rc;
        d_frames_bgr = adas::remap_frames(p->remap);
    }
    if (!p->det_in && !p->lane_in) {
        const char* env = getenv("ADAS_NO_PACKED_SEAM");
        p->packed = !(env && env[0] == '1') && (!p->d.detector || adas_engine_accepts_packed_input(p->d.detector)) &&
                    (!p->d.lane || adas_engine_accepts_packed_input(p->d.lane));
    }
    if (p->d.detector && !p->det_in) {
        int64_t is[4];
        adas_engine_input_shape(p->d.detector, is);
        ADAS_HIP_TRY(hipMalloc((void**)&p->det_in, S * (size_t)(is[1] * is[2] * is[3]) * 4));
    }
    if (p->d.lane && !p->lane_in) {
        int64_t is[4];
        adas_engine_input_shape(p->d.lane, is);
        ADAS_HIP_TRY(hipMalloc((void**)&p->lane_in, S * (size_t)(is[1] * is[2] * is[3]) * 4));
    }
    const adas_pipeline::FrameSrc fs{d_frames_bgr, src_h, src_w, lane_crop_ratio};
    if (!(p->d.use_graph & 1)) {
        p->fsrc = fs;
        p->timed = true;
        int rc = record_step(p, p->det_in, p->lane_in, true);
        p->fsrc.frames = nullptr;
        return rc;
    }
    return replay_step(p, adas_pipeline::GraphKey{d_frames_bgr, nullptr, src_h, src_w, lane_crop_ratio}, p->det_in, p->lane_in, &fs);
}

int adas_pipeline_step_frames_host(adas_pipeline* p, const uint8_t* h_frames_bgr, int src_h, int src_w, double lane_crop_ratio) {
    ADAS_REQUIRE(p && h_frames_bgr && src_h > 0 && src_w > 0, ADAS_ERR_INVALID, "adas_pipeline_step_frames_host: bad argument");
    const size_t bytes = (size_t)p->d.n_streams * (p->d.micro_batch > 1 ? p->d.micro_batch : 1) * src_h * src_w * 3;
    if (!p->st_copy) ADAS_HIP_TRY(hipStreamCreateWithFlags(&p->st_copy, hipStreamNonBlocking));
    if (!p->ev_copied[0]) {
        for (int k = 0; k < 2; ++k) {
            ADAS_HIP_TRY(hipEventCreateWithFlags(&p->ev_copied[k], hipEventDisableTiming));
            ADAS_HIP_TRY(hipEventCreateWithFlags(&p->ev_consumed[k], hipEventDisableTiming));
        }
    }
    if (bytes > p->host_stage_bytes) {  // (re)size both staging buffers; captured steps that read the old ones are dropped
        ADAS_HIP_TRY(hipStreamSynchronize(p->st));
        ADAS_HIP_TRY(hipStreamSynchronize(p->st_copy));
        drop_graphs(p);
        for (int k = 0; k < 2; ++k) {
            if (p->host_stage[k]) (void)hipFree(p->host_stage[k]);
            p->host_stage[k] = nullptr;
            ADAS_HIP_TRY(hipMalloc((void**)&p->host_stage[k], bytes));
        }
        p->host_stage_bytes = bytes;
        p->host_steps = 0;
    }
    const int k = (int)(p->host_steps & 1);
    if (p->host_steps >= 2) ADAS_HIP_TRY(hipStreamWaitEvent(p->st_copy, p->ev_consumed[k], 0));  // the step two back is done with buffer k
    ADAS_HIP_TRY(hipMemcpyAsync(p->host_stage[k], h_frames_bgr, bytes, hipMemcpyHostToDevice, p->st_copy));
    ADAS_HIP_TRY(hipEventRecord(p->ev_copied[k], p->st_copy));
    ADAS_HIP_TRY(hipStreamWaitEvent(p->st, p->ev_copied[k], 0));
    int rc = adas_pipeline_step_frames(p, p->host_stage[k], src_h, src_w, lane_crop_ratio);
    if (rc) return rc;
    ADAS_HIP_TRY(hipEventRecord(p->ev_consumed[k], p->st));
    ++p->host_steps;
    return ADAS_OK;
}

int adas_pipeline_wait_upload(adas_pipeline* p) {
    ADAS_REQUIRE(p, ADAS_ERR_INVALID, "null pipeline");
    if (p->st_copy) ADAS_HIP_TRY(hipStreamSynchronize(p->st_copy));
    return ADAS_OK;
}

int adas_pipeline_attach_scale(adas_pipeline* p, adas_scale* scale, int source) {
    ADAS_REQUIRE(p, ADAS_ERR_INVALID, "adas_pipeline_attach_scale: null pipeline");
    if (scale) {
        ADAS_REQUIRE(source == ADAS_SCALE_SRC_OVERLAY || source == ADAS_SCALE_SRC_FRAMES, ADAS_ERR_INVALID, "adas_pipeline_attach_scale: unknown source %d",
                     source);
        ADAS_REQUIRE(source != ADAS_SCALE_SRC_OVERLAY || p->overlay, ADAS_ERR_INVALID,
                     "adas_pipeline_attach_scale: the overlay source needs an attached overlay handle (adas_pipeline_attach_overlay first)");
        const int frames = p->d.n_streams * (p->d.micro_batch > 1 ? p->d.micro_batch : 1);
        int sw = 0, sh = 0, cw = 0, ch = 0, tiles = 0, sb = 0, border = 0;
        adas::scale_geometry_of(scale, &sw, &sh, &cw, &ch, &tiles, &sb, &border);
        ADAS_REQUIRE(sb >= frames, ADAS_ERR_INVALID, "adas_pipeline_attach_scale: the scale handle holds %d frames, a step has %d", sb, frames);
        ADAS_REQUIRE(border == 0 || p->analysis, ADAS_ERR_INVALID,
                     "adas_pipeline_attach_scale: a border of %d pixels needs an attached analysis handle (adas_pipeline_attach_analysis first)", border);
        if (border > 0) {
            int af = 0;
            ADAS_REQUIRE(adas::analysis_capacity(p->analysis, nullptr, &af) && frames <= af, ADAS_ERR_INVALID,
                         "adas_pipeline_attach_scale: a step has %d frames, the analysis handle holds %d", frames, af);
        }
        if (source == ADAS_SCALE_SRC_OVERLAY) {
            int oh = 0, ow = 0, obh = 0, obw = 0, ob = 0;
            (void)adas::overlay_geometry(p->overlay, &oh, &ow, &obh, &obw, &ob);
            ADAS_REQUIRE(oh == sh && ow == sw, ADAS_ERR_INVALID,
                         "adas_pipeline_attach_scale: the scale handle was created for %dx%d frames, the attached overlay draws %dx%d", sw, sh, ow, oh);
        }
    }
    ADAS_HIP_TRY(hipStreamSynchronize(p->st));
    drop_graphs(p);
    p->scale = scale;
    p->scale_source = source;
    p->scale_jpeg = nullptr;   // the canvases' encoders were checked against the handle that leaves: they are attached again behind a new one
    p->scale_yuvout = nullptr;
    return ADAS_OK;
}

// what both consumers of the canvases check: a handle for `held` frames of w x h against the attached scale handle
static int scale_consumer_check(const char* who, const char* what, adas_pipeline* p, int w, int h, int held) {
    ADAS_REQUIRE(p->scale, ADAS_ERR_INVALID, "%s: no scale handle is attached (adas_pipeline_attach_scale first)", who);
    const int frames = p->d.n_streams * (p->d.micro_batch > 1 ? p->d.micro_batch : 1);
    int sw = 0, sh = 0, cw = 0, ch = 0, tiles = 0, sb = 0, border = 0;
    adas::scale_geometry_of(p->scale, &sw, &sh, &cw, &ch, &tiles, &sb, &border);
    ADAS_REQUIRE(w == cw && h == ch, ADAS_ERR_INVALID, "%s: the %s handle was created for %dx%d frames, the scale handle's canvas is %dx%d", who, what, w, h,
                 cw, ch);
    const int canvases = (frames + tiles - 1) / tiles;
    ADAS_REQUIRE(held >= canvases, ADAS_ERR_INVALID, "%s: the %s handle holds %d frames, a step has %d canvases", who, what, held, canvases);
    return ADAS_OK;
}

int adas_pipeline_attach_scale_jpeg(adas_pipeline* p, adas_jpeg* jpeg) {
    ADAS_REQUIRE(p, ADAS_ERR_INVALID, "adas_pipeline_attach_scale_jpeg: null pipeline");
    if (jpeg) {
        int jw = 0, jh = 0, jb = 0;
        adas::jpeg_geometry_of(jpeg, &jw, &jh, &jb);
        const int rc = scale_consumer_check("adas_pipeline_attach_scale_jpeg", "JPEG", p, jw, jh, jb);
        if (rc) return rc;
    }
    ADAS_HIP_TRY(hipStreamSynchronize(p->st));
    drop_graphs(p);
    p->scale_jpeg = jpeg;
    return ADAS_OK;
}

int adas_pipeline_attach_scale_yuvout(adas_pipeline* p, adas_yuvout* yuvout) {
    ADAS_REQUIRE(p, ADAS_ERR_INVALID, "adas_pipeline_attach_scale_yuvout: null pipeline");
    if (yuvout) {
        int yw = 0, yh = 0, yb = 0;
        adas::yuvout_geometry_of(yuvout, &yw, &yh, &yb);
        const int rc = scale_consumer_check("adas_pipeline_attach_scale_yuvout", "YUV output", p, yw, yh, yb);
        if (rc) return rc;
    }
    ADAS_HIP_TRY(hipStreamSynchronize(p->st));
    drop_graphs(p);
    p->scale_yuvout = yuvout;
    return ADAS_OK;
}

int adas_pipeline_attach_jpegdec(adas_pipeline* p, adas_jpegdec* jpegdec) {
    ADAS_REQUIRE(p, ADAS_ERR_INVALID, "adas_pipeline_attach_jpegdec: null pipeline");
    if (jpegdec) {
        const int frames = p->d.n_streams * (p->d.micro_batch > 1 ? p->d.micro_batch : 1);
        int jw = 0, jh = 0, jb = 0;
        adas::jpegdec_geometry_of(jpegdec, &jw, &jh, &jb);
        ADAS_REQUIRE(jb >= frames, ADAS_ERR_INVALID, "adas_pipeline_attach_jpegdec: the decoder handle holds %d frames, a step has %d", jb, frames);
    }
    ADAS_HIP_TRY(hipStreamSynchronize(p->st));
    if (p->st_copy) ADAS_HIP_TRY(hipStreamSynchronize(p->st_copy));
    p->jpegdec = jpegdec;
    p->jslot_used[0] = p->jslot_used[1] = false;
    return ADAS_OK;
}

int adas_pipeline_step_jpeg_host(adas_pipeline* p, const uint8_t* const* h_streams, const int64_t* h_lengths, double lane_crop_ratio) {
    ADAS_REQUIRE(p && h_streams && h_lengths, ADAS_ERR_INVALID, "adas_pipeline_step_jpeg_host: bad argument");
    ADAS_REQUIRE(p->jpegdec, ADAS_ERR_INVALID, "adas_pipeline_step_jpeg_host: no decoder handle attached (adas_pipeline_attach_jpegdec first)");
    const int frames = p->d.n_streams * (p->d.micro_batch > 1 ? p->d.micro_batch : 1);
    int jw = 0, jh = 0, jb = 0;
    adas::jpegdec_geometry_of(p->jpegdec, &jw, &jh, &jb);
    if (!p->st_copy) ADAS_HIP_TRY(hipStreamCreateWithFlags(&p->st_copy, hipStreamNonBlocking));
    for (int k = 0; k < 2; ++k)
        if (!p->ev_jcopied[k]) {
            ADAS_HIP_TRY(hipEventCreateWithFlags(&p->ev_jcopied[k], hipEventDisableTiming));
            ADAS_HIP_TRY(hipEventCreateWithFlags(&p->ev_jconsumed[k], hipEventDisableTiming));
        }
    // the slot the decoder packs into alternates with every call: the copy waits only for the decode that last read that slot (two steps
    // back), so it runs under the previous step's decode and nets
    const int next = adas::jpegdec_next_slot(p->jpegdec);
    if (p->jslot_used[next]) ADAS_HIP_TRY(hipStreamWaitEvent(p->st_copy, p->ev_jconsumed[next], 0));
    int slot = next;
    int rc = adas::jpegdec_stage_host(p->jpegdec, h_streams, h_lengths, frames, p->st_copy, &slot);
    if (rc) return rc;
    ADAS_REQUIRE(slot == next, ADAS_ERR_INVALID, "adas_pipeline_step_jpeg_host: the decoder's staging slot moved under the step");
    ADAS_HIP_TRY(hipEventRecord(p->ev_jcopied[slot], p->st_copy));
    ADAS_HIP_TRY(hipStreamWaitEvent(p->st, p->ev_jcopied[slot], 0));
    rc = adas::jpegdec_run_slot(p->jpegdec, slot, frames, nullptr, p->st);
    if (rc) return rc;
    ADAS_HIP_TRY(hipEventRecord(p->ev_jconsumed[slot], p->st));
    p->jslot_used[slot] = true;
    return adas_pipeline_step_frames(p, adas::jpegdec_frames(p->jpegdec), jh, jw, lane_crop_ratio);
}

int adas_pipeline_attach_yuv(adas_pipeline* p, adas_yuv* yuv) {
    ADAS_REQUIRE(p, ADAS_ERR_INVALID, "adas_pipeline_attach_yuv: null pipeline");
    if (yuv) {
        const int frames = p->d.n_streams * (p->d.micro_batch > 1 ? p->d.micro_batch : 1);
        int yw = 0, yh = 0, yb = 0;
        long long ys = 0;
        adas::yuv_geometry_of(yuv, &yw, &yh, &yb, &ys);
        ADAS_REQUIRE(yb >= frames, ADAS_ERR_INVALID, "adas_pipeline_attach_yuv: the conversion handle holds %d frames, a step has %d", yb, frames);
    }
    ADAS_HIP_TRY(hipStreamSynchronize(p->st));
    if (p->st_copy) ADAS_HIP_TRY(hipStreamSynchronize(p->st_copy));
    p->yuv = yuv;
    p->yuv_steps = 0;
    return ADAS_OK;
}

int adas_pipeline_step_yuv(adas_pipeline* p, const uint8_t* d_src, double lane_crop_ratio) {
    ADAS_REQUIRE(p && d_src, ADAS_ERR_INVALID, "adas_pipeline_step_yuv: bad argument");
    ADAS_REQUIRE(p->yuv, ADAS_ERR_INVALID, "adas_pipeline_step_yuv: no conversion handle attached (adas_pipeline_attach_yuv first)");
    const int frames = p->d.n_streams * (p->d.micro_batch > 1 ? p->d.micro_batch : 1);
    int yw = 0, yh = 0, yb = 0;
    long long ys = 0;
    adas::yuv_geometry_of(p->yuv, &yw, &yh, &yb, &ys);
    int rc = adas_yuv_run(p->yuv, d_src, frames, nullptr, p->st);
    if (rc) return rc;
    return adas_pipeline_step_frames(p, adas::yuv_frames(p->yuv), yh, yw, lane_crop_ratio);
}

int adas_pipeline_step_yuv_host(adas_pipeline* p, const uint8_t* h_src, double lane_crop_ratio) {
    ADAS_REQUIRE(p && h_src, ADAS_ERR_INVALID, "adas_pipeline_step_yuv_host: bad argument");
    ADAS_REQUIRE(p->yuv, ADAS_ERR_INVALID, "adas_pipeline_step_yuv_host: no conversion handle attached (adas_pipeline_attach_yuv first)");
    const int frames = p->d.n_streams * (p->d.micro_batch > 1 ? p->d.micro_batch : 1);
    int yw = 0, yh = 0, yb = 0;
    long long ys = 0;
    adas::yuv_geometry_of(p->yuv, &yw, &yh, &yb, &ys);
    const size_t bytes = (size_t)frames * (size_t)ys;
    if (!p->st_copy) ADAS_HIP_TRY(hipStreamCreateWithFlags(&p->st_copy, hipStreamNonBlocking));
    for (int k = 0; k < 2; ++k)
        if (!p->ev_ycopied[k]) {
            ADAS_HIP_TRY(hipEventCreateWithFlags(&p->ev_ycopied[k], hipEventDisableTiming));
            ADAS_HIP_TRY(hipEventCreateWithFlags(&p->ev_yconsumed[k], hipEventDisableTiming));
        }
    if (bytes > p->yuv_stage_bytes) {  // (re)size both staging buffers; no captured step reads them
        ADAS_HIP_TRY(hipStreamSynchronize(p->st));
        ADAS_HIP_TRY(hipStreamSynchronize(p->st_copy));
        for (int k = 0; k < 2; ++k) {
            if (p->yuv_stage[k]) (void)hipFree(p->yuv_stage[k]);
            p->yuv_stage[k] = nullptr;
            ADAS_HIP_TRY(hipMalloc((void**)&p->yuv_stage[k], bytes));
        }
        p->yuv_stage_bytes = bytes;
        p->yuv_steps = 0;
    }
    const int k = (int)(p->yuv_steps & 1);
    if (p->yuv_steps >= 2) ADAS_HIP_TRY(hipStreamWaitEvent(p->st_copy, p->ev_yconsumed[k], 0));  // the conversion two steps back is done with buffer k
    // the last frame is read up to the end of its last plane only: the host need not hold a whole frame_stride behind it
    ADAS_HIP_TRY(hipMemcpyAsync(p->yuv_stage[k], h_src, bytes - (size_t)ys + (size_t)adas::yuv_extent_of(p->yuv), hipMemcpyHostToDevice, p->st_copy));
    ADAS_HIP_TRY(hipEventRecord(p->ev_ycopied[k], p->st_copy));
    ADAS_HIP_TRY(hipStreamWaitEvent(p->st, p->ev_ycopied[k], 0));
    int rc = adas_yuv_run(p->yuv, p->yuv_stage[k], frames, nullptr, p->st);
    if (rc) return rc;
    ADAS_HIP_TRY(hipEventRecord(p->ev_yconsumed[k], p->st));   // the conversion alone reads the buffer: the next copy into it need not wait for the step
    ++p->yuv_steps;
    return adas_pipeline_step_frames(p, adas::yuv_frames(p->yuv), yh, yw, lane_crop_ratio);
}

int adas_pipeline_attach_remap(adas_pipeline* p, adas_remap* remap) {
    ADAS_REQUIRE(p, ADAS_ERR_INVALID, "adas_pipeline_attach_remap: null pipeline");
    if (remap) {
        const int frames = p->d.n_streams * (p->d.micro_batch > 1 ? p->d.micro_batch : 1);
        int sh = 0, sw = 0, dh = 0, dw = 0, ns = 0, rb = 0;
        adas::remap_geometry_of(remap, &sh, &sw, &dh, &dw, &ns, &rb);
        ADAS_REQUIRE(sh == dh && sw == dw, ADAS_ERR_INVALID,
                     "adas_pipeline_attach_remap: the step reads frames of the size it is given: the remap handle turns %dx%d into %dx%d", sw, sh, dw, dh);
        ADAS_REQUIRE(ns == p->d.n_streams, ADAS_ERR_INVALID, "adas_pipeline_attach_remap: the remap handle was created for %d streams, the pipeline has %d", ns,
                     p->d.n_streams);
        ADAS_REQUIRE(rb >= frames, ADAS_ERR_INVALID, "adas_pipeline_attach_remap: the remap handle holds %d frames, a step has %d", rb, frames);
        const uint8_t* own = nullptr;   // the buffer the captured step will read exists from here on
        int rc = adas_remap_device_view(remap, &own);
        if (rc) return rc;
    }
    ADAS_HIP_TRY(hipStreamSynchronize(p->st));
    drop_graphs(p);
    if (p->remap) adas::remap_forget_stream(p->remap);   // the handle that leaves has drained: its fetches no longer need this pipeline's stream
    p->remap = remap;
    return ADAS_OK;
}

int adas_pipeline_sync(adas_pipeline* p) {
    ADAS_REQUIRE(p, ADAS_ERR_INVALID, "null pipeline");
    ADAS_HIP_TRY(hipStreamSynchronize(p->st));
    // engines running the opt-in multi-layer launches (ADAS_ML=1) report a timed-out dependency wait here: the step's results are then
    // incomplete and the caller must not use them (adas_engine_ml_status returns at once for every other engine)
    const int frames = p->d.n_streams * (p->d.micro_batch > 1 ? p->d.micro_batch : 1);
    for (adas_engine* e : {p->d.detector, p->d.lane})
        if (e) {
            uint32_t w = 0;
            int rc = adas_engine_ml_status(e, frames, &w);
            if (rc != ADAS_OK) return rc;
        }
    return ADAS_OK;
}

int adas_pipeline_timings(adas_pipeline* p, float ms[6]) {
    ADAS_REQUIRE(p && ms, ADAS_ERR_INVALID, "null argument");
    ADAS_HIP_TRY(hipStreamSynchronize(p->st));
    for (int i = 0; i < 6; ++i) ms[i] = 0.f;
    ADAS_HIP_TRY(hipEventElapsedTime(&ms[5], p->ev[0], p->ev[5]));
    if (p->timed)
        for (int i = 0; i < 5; ++i) ADAS_HIP_TRY(hipEventElapsedTime(&ms[i], p->ev[i], p->ev[i + 1]));
    return ADAS_OK;
}
}
