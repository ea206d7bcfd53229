// engine.cpp -- HipEngine: runs a loaded ADASHIP1 model (engine_load.cpp: adas_engine_create) on one MI355X.
// Replaces EngineBase / OnnxEngine / TensorRTEngine (coreEngine.py:7-39,120-186): same surface
// (input shape, output shapes+names, inference on an NCHW tensor), plus a device-resident form.
#include "engine.h"
#include <errno.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

using namespace adas;

// is op `i` one of the three convs a fused C2f launch computes besides its cv1?
static bool in_c2f(const adas_engine* e, int i) {
    for (auto& q : e->ops)
        if (q.c2f[0] == i || q.c2f[1] == i || q.c2f[2] == i) return true;
    return false;
}

static bool is_c2f_tail(const adas_engine* e, int i) {   // the block's cv2: its output IS materialised
    for (auto& q : e->ops)
        if (q.c2f[2] == i) return true;
    return false;
}

// The ConvArgs of op `i` (a plain OP_CONV: not a stem / pair / C2f launch) at this batch, without a folded projection shortcut (fold_ds).
static ConvArgs conv_args_of(const adas_engine* e, int i, int batch) {
    const EngOp& op = e->ops[i];
    const FileOp& o = op.f;
    unsigned char* wb = (unsigned char*)e->d_weights;
    ConvArgs a;
    a.in = make_view(e, o.in_buf[0], o.in_coff[0], o.in_c[0]);
    a.out = make_view(e, o.out_buf, o.out_coff, o.out_c);
    if (o.res_mode != RES_NONE) a.res = make_view(e, o.res_buf, o.res_coff, o.out_c);
    else { a.res = a.out; a.res.p = nullptr; }
    a.wgt = wb + op.w_off;
    a.bias = (const float*)(wb + op.b_off);
    a.n = batch; a.kh = o.kh; a.kw = o.kw; a.stride = o.stride; a.pad = o.pad; a.act = o.act; a.res_mode = o.res_mode;
    a.k = op.k; a.kpad = op.kpad; a.m = batch * a.out.h * a.out.w; a.max_n = e->max_batch; a.prec = e->prec;
    if (op.has_x3h8) a.wgt_h8x3 = wb + op.x3h8_w_off;
    a.halo_bn = op.halo_bn;
    if (op.up_src >= 0) {
        const FileOp& u = e->ops[op.up_src].f;
        a.up = make_view(e, u.in_buf[0], u.in_coff[0], u.in_c[0]);
        a.up_c = (int)u.out_c;
    }
    return a;
}

// `a` = conv_args_of(e, i, batch): does the launch take the conv's projection shortcut (if it has a link to one) into itself?  Only conv_h8
// computes it, so: where the conv runs on conv_h8 as it is (asked with its real residual view, the projection's output buffer) and conv_h8
// can carry this projection.  Then the projection's arguments are added to `a`.
static bool fold_ds(const adas_engine* e, int i, ConvArgs* a) {
    if (e->ops[i].ds_src < 0 || e->ops[i].kernel != CONV_HALO) return false;
    const EngOp& dsop = e->ops[e->ops[i].ds_src];
    const TView x = make_view(e, dsop.f.in_buf[0], dsop.f.in_coff[0], dsop.f.in_c[0]);
    if (conv_route(*a) != ConvRoute::H8 || !halo8_ds_applicable(*a, x)) return false;
    unsigned char* wb = (unsigned char*)e->d_weights;
    a->ds_in = x;
    a->ds_w = wb + dsop.ds_w_off;
    a->ds_bias = (const float*)(wb + dsop.b_off);
    return true;
}

// does conv `ci` (with a projection shortcut link) take its shortcut into its own launch at this batch?
static bool ds_folded(const adas_engine* e, int ci, int batch) {
    if (e->ops[ci].ds_src < 0) return false;
    ConvArgs a = conv_args_of(e, ci, batch);
    return fold_ds(e, ci, &a);
}

// ---- multi-layer launches (conv_ml.hip): opt-in, ADAS_ML=1 when the engine is created.
static bool ml_enabled(const adas_engine* e) { return e->ml_on; }   // decided when the engine was created (ADAS_ML=1, 16-bit precisions)

// Is op `i` a conv that launches on its own at this batch AND has a tile body in the multi-layer kernel?
static bool ml_candidate(const adas_engine* e, int i, int batch, ConvArgs* out) {
    const EngOp& op = e->ops[i];
    const FileOp& o = op.f;
    if (o.type != OP_CONV || op.skip || (op.kernel != CONV_HALO && op.kernel != CONV_PW)) return false;
    if (op.pair_b >= 0 || op.c2f[0] >= 0 || op.fuse_pool >= 0 || op.fuse_conv2 >= 0) return false;
    if (op.ds_user >= 0 && ds_folded(e, op.ds_user, batch)) return false;   // launches nothing at this batch
    if (op.ds_src >= 0 && ds_folded(e, i, batch)) return false;              // carries its projection: conv_halo8 only
    auto aliased = [&](int b) { return b >= 0 && b < (int)e->buf_aliased.size() && e->buf_aliased[b]; };
    if (aliased(o.in_buf[0]) || aliased(o.out_buf) || (o.res_mode != RES_NONE && aliased(o.res_buf))) return false;
    if (op.up_src >= 0 && aliased(e->ops[op.up_src].f.in_buf[0])) return false;
    {   // experiments: ADAS_ML_ONLY=halo | pw keeps the other kind of layer out of the launches
        const char* only = getenv("ADAS_ML_ONLY");
        if (only && ((only[0] == 'h' && op.kernel != CONV_HALO) || (only[0] == 'p' && op.kernel != CONV_PW))) return false;
    }
    const ConvArgs a = conv_args_of(e, i, batch);
    if (!ml_layer_supported(a, op.kernel)) return false;
    if (out) *out = a;
    return true;
}

// Is op `i` a 3x3 conv that launches on conv_halo at this batch (a layer the grouped launch can carry)?
static bool group_candidate(const adas_engine* e, int i, int batch, ConvArgs* out) {
    const EngOp& op = e->ops[i];
    const FileOp& o = op.f;
    if (o.type != OP_CONV || op.skip || op.kernel != CONV_HALO) return false;
    if (op.pair_b >= 0 || op.c2f[0] >= 0 || op.fuse_pool >= 0 || op.fuse_conv2 >= 0 || op.up_src >= 0) return false;
    if (op.ds_user >= 0 && ds_folded(e, op.ds_user, batch)) return false;
    if (op.ds_src >= 0 && ds_folded(e, i, batch)) return false;
    auto aliased = [&](int b) { return b >= 0 && b < (int)e->buf_aliased.size() && e->buf_aliased[b]; };
    if (aliased(o.in_buf[0]) || aliased(o.out_buf) || (o.res_mode != RES_NONE && aliased(o.res_buf))) return false;
    const ConvArgs a = conv_args_of(e, i, batch);
    if (!group_layer_supported(a, op.kernel)) return false;
    if (out) *out = a;
    return true;
}

static const std::vector<GroupRun>* group_runs(const adas_engine* e, int batch) {
    auto it = e->groups.find(batch);
    return it == e->groups.end() ? nullptr : &it->second;
}

static const std::vector<MlSeg>* ml_segments(const adas_engine* e, int batch) {
    auto it = e->ml.find(batch);
    return it == e->ml.end() ? nullptr : &it->second;
}

int adas::free_engine(adas_engine* e) {
    if (!e) return ADAS_OK;
    for (auto& kv : e->ml)
        for (auto& sg : kv.second) ml_plan_destroy(sg.plan);
    e->ml.clear();
    for (auto& kv : e->groups)
        for (auto& run : kv.second)
            for (auto& st : run.steps) ml_group_destroy(st.group);
    e->groups.clear();
    for (auto& b : e->bufs)
        if (b.d && b.alias_of < 0) (void)hipFree(b.d);
    if (e->d_weights) (void)hipFree(e->d_weights);
    if (e->d_input) (void)hipFree(e->d_input);
    for (auto& ev : e->events)
        if (ev) (void)hipEventDestroy(ev);
    for (auto& ev : e->step_events)
        if (ev) (void)hipEventDestroy(ev);
    delete e;
    return ADAS_OK;
}

extern "C" {

int adas_engine_destroy(adas_engine* e) { return free_engine(e); }

int adas_engine_input_shape(const adas_engine* e, int64_t dims[4]) {
    ADAS_REQUIRE(e && dims, ADAS_ERR_INVALID, "null argument");
    dims[0] = 1; dims[1] = e->hdr.in_c; dims[2] = e->hdr.in_h; dims[3] = e->hdr.in_w;
    return ADAS_OK;
}
int adas_engine_num_outputs(const adas_engine* e) { return e ? (int)e->outs.size() : 0; }
int adas_engine_output_shape(const adas_engine* e, int index, int64_t dims[4], int* ndim) {
    ADAS_REQUIRE(e && dims && ndim && index >= 0 && index < (int)e->outs.size(), ADAS_ERR_INVALID, "bad output index");
    for (int i = 0; i < 4; ++i) dims[i] = e->outs[index].dims[i];
    *ndim = e->outs[index].ndim;
    return ADAS_OK;
}
const char* adas_engine_output_name(const adas_engine* e, int index) {
    if (!e || index < 0 || index >= (int)e->outs.size()) return "";
    return e->outs[index].name.c_str();
}
int adas_engine_stats(const adas_engine* e, double* flops, double* wbytes, int* nl) {
    ADAS_REQUIRE(e, ADAS_ERR_INVALID, "null engine");
    if (flops) *flops = e->hdr.flops;
    if (wbytes) *wbytes = (double)e->weight_bytes;
    if (nl) *nl = (int)e->ops.size();
    return ADAS_OK;
}
int adas_engine_layer_kernel(const adas_engine* e, int layer, int batch, char* name, int cap) {
    ADAS_REQUIRE(e && name && cap > 0 && layer >= 0 && layer < (int)e->ops.size() && batch > 0, ADAS_ERR_INVALID, "bad layer index");
    const EngOp& op = e->ops[layer];
    const FileOp& o = op.f;
    static const char* kOther[] = {"input_nchw_kernel", "", "maxpool_kernel", "upsample2_kernel", "detect_v8_kernel", "detect_v5_kernel",
                                   "layernorm_kernel", "dwconv_kernel", "attention_kernel", "avgpool_kernel", "depth2space_kernel", "detect_v6_kernel",
                                   "se_gate_kernel", "scale_kernel", "wsum_kernel", "shuffle_kernel"};
    const MlSeg* in_seg = nullptr;
    if (const std::vector<MlSeg>* segs = ml_segments(e, batch))
        for (auto& sg : *segs)
            for (int m : sg.ops)
                if (m == layer) in_seg = &sg;
    const GroupRun* in_run = nullptr;
    if (const std::vector<GroupRun>* runs = group_runs(e, batch))
        for (auto& run : *runs)
            for (int m : run.ops)
                if (m == layer) in_run = &run;
    // a layer of a run belongs to one STEP of it: a grouped launch (its first member carries the label, the others ride in it) or a
    // single layer on its own kernel, which is labelled like any other layer below
    const GroupStep* in_step = nullptr;
    if (in_run)
        for (auto& st : in_run->steps)
            for (int m : st.members)
                if (m == layer) in_step = &st;
    if (in_step && in_step->group && in_step->members.front() == layer) {
        snprintf(name, cap, "conv_halo_group_kernel[%d layers]", (int)in_step->members.size());
    } else if (in_step && in_step->group) {
        snprintf(name, cap, "(in the grouped launch)");
    } else if (in_seg && in_seg->first == layer) {
        snprintf(name, cap, "conv_ml_kernel[%d layers]", in_seg->n_layers);
    } else if (in_seg) {
        snprintf(name, cap, "(in the multi-layer launch)");
    } else if (o.type == OP_CONV && op.ds_user >= 0 && ds_folded(e, op.ds_user, batch)) {
        snprintf(name, cap, "(fused into the conv it is the shortcut of)");
    } else if (op.skip && o.type == OP_UPSAMPLE2) {
        snprintf(name, cap, "(folded into the consumer's loads)");
    } else if (op.skip && o.type == OP_MAXPOOL && (o.kh == 5 || o.kh == 9 || o.kh == 13)) {
        snprintf(name, cap, "(fused into the SPPF pool launch)");
    } else if (o.type == OP_MAXPOOL && op.pool3[0] >= 0) {
        snprintf(name, cap, "sppf_pool3_kernel");
    } else if (o.type == OP_CONV && op.c2f[0] >= 0) {
        snprintf(name, cap, e->prec == PREC_X3 ? "conv_c2f16_x3_kernel" : "conv_c2f16_kernel");
    } else if (op.skip && o.type == OP_CONV && in_c2f(e, layer)) {
        snprintf(name, cap, "(fused into the C2f launch)");
    } else if (op.skip && op.kernel == CONV_PAIR) {
        snprintf(name, cap, "(fused into the pair launch)");
    } else if (o.type == OP_CONV && op.pair_b >= 0) {
        snprintf(name, cap, "conv_pair_kernel<%d>", (int)o.out_c);
    } else if (op.skip) {
        snprintf(name, cap, o.type == OP_CONV && o.kh == 1 && (op.kernel == CONV_PW || op.kernel == CONV_DET5) ? "(fused into the Detect launch)" : "(fused into the stem launch)");
    } else if (o.type == OP_CONV && op.kernel == CONV_STEM && op.fuse_conv2 >= 0) {
        snprintf(name, cap, e->prec == PREC_X3 ? "conv_stem2_x3_kernel<%d>+conv3x3s2" : "conv_stem_kernel<%d,1,SILU>+conv3x3s2", (int)o.kh);
    } else if (o.type == OP_CONV) {
        ConvArgs a = conv_args_of(e, layer, batch);
        const bool shortcut = fold_ds(e, layer, &a);
        snprintf(name, cap, "%s%s%s", conv_kernel_name(a, op.kernel == CONV_STEM), op.fuse_pool >= 0 ? "+pool" : "", shortcut ? "+shortcut" : "");
    } else if (o.type == OP_DETECT_V8 && op.det_src[0] >= 0) {
        snprintf(name, cap, e->prec == PREC_X3 ? "detect_v8_fused_x3_kernel" : "detect_v8_fused_kernel");
    } else if (o.type == OP_DETECT_V5 && op.det_src[0] >= 0) {
        snprintf(name, cap, "detect_v5_fused_kernel");
    } else if (o.type == OP_DETECT_V6 && o.params[5] != 0.0f) {
        snprintf(name, cap, "detect_v6_dfl_kernel");
    } else {
        snprintf(name, cap, "%s", o.type < 16 ? kOther[o.type] : "?");
    }
    return ADAS_OK;
}
int adas_engine_detect_sink_supported(const adas_engine* e) {
    if (!e) return 0;
    for (auto& op : e->ops)
        if ((op.f.type == OP_DETECT_V8 || op.f.type == OP_DETECT_V5) && op.det_src[0] >= 0) return 1;
    return 0;
}
int adas_engine_detect_sink_shape(const adas_engine* e, int32_t* layout, int32_t* num_anchors, int32_t* num_classes) {
    ADAS_REQUIRE(e, ADAS_ERR_INVALID, "adas_engine_detect_sink_shape: null engine");
    for (auto& op : e->ops)
        if ((op.f.type == OP_DETECT_V8 || op.f.type == OP_DETECT_V5) && op.det_src[0] >= 0) {
            if (layout) *layout = op.f.type == OP_DETECT_V8 ? ADAS_HEAD_V8 : ADAS_HEAD_V5;
            if (num_classes) *num_classes = (int32_t)op.f.params[0];
            if (num_anchors) *num_anchors = (int32_t)op.f.params[1];
            return ADAS_OK;
        }
    set_error("this engine has no fused Detect kernel");
    return ADAS_ERR_INVALID;
}
int adas_engine_set_detect_sink(adas_engine* e, float* d_best_conf, int32_t* d_best_cls) {
    ADAS_REQUIRE(e && ((d_best_conf == nullptr) == (d_best_cls == nullptr)), ADAS_ERR_INVALID, "adas_engine_set_detect_sink: bad argument");
    ADAS_REQUIRE(!d_best_conf || adas_engine_detect_sink_supported(e), ADAS_ERR_INVALID,
                 "this engine's Detect is not one of the fused kernels (16-bit precisions, the head's last 1x1 convs folded in): it has no per-anchor sink");
    e->sink_conf = d_best_conf;
    e->sink_cls = d_best_cls;
    return ADAS_OK;
}
int adas_engine_layer_info(const adas_engine* e, int layer, char* name, int cap, double* flops, int* kind) {
    ADAS_REQUIRE(e && layer >= 0 && layer < (int)e->ops.size(), ADAS_ERR_INVALID, "bad layer index");
    if (name && cap > 0) snprintf(name, cap, "%s", e->ops[layer].name.c_str());
    if (flops) *flops = e->ops[layer].f.flops;
    if (kind) *kind = (int)e->ops[layer].f.type;
    return ADAS_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------- execution
namespace adas {

int engine_run_op(adas_engine* e, int i, const float* d_in, int batch, hipStream_t st, bool packed_in) {
    EngOp& op = e->ops[i];
    const FileOp& o = op.f;
    unsigned char* wb = (unsigned char*)e->d_weights;
    hipError_t err = hipSuccess;
    if (op.skip) return ADAS_OK;  // folded into the stem launch
    if (o.type == OP_CONV && op.kernel == CONV_STEM) {
        TView cv = make_view(e, o.out_buf, o.out_coff, o.out_c);
        TView pv = cv;
        if (op.fuse_pool >= 0) {
            const FileOp& po = e->ops[op.fuse_pool].f;
            pv = make_view(e, po.out_buf, po.out_coff, po.out_c);
        }
        if (e->prec == PREC_X3 && op.fuse_conv2 >= 0) {
            const EngOp& c2 = e->ops[op.fuse_conv2];
            err = launch_conv_stem2_x3(d_in, batch, e->hdr.in_c, e->hdr.in_h, e->hdr.in_w, o.kh, o.pad, wb + op.w_off, (const float*)(wb + op.b_off), cv,
                                       wb + c2.w_off, (const float*)(wb + c2.b_off), make_view(e, c2.f.out_buf, c2.f.out_coff, c2.f.out_c), st);
        } else if (e->prec == PREC_X3 && op.fuse_pool >= 0) {
            err = launch_conv_stem_pool_x3(d_in, batch, e->hdr.in_c, e->hdr.in_h, e->hdr.in_w, o.pad, wb + op.w_off, (const float*)(wb + op.b_off), cv, pv, st);
        } else if (e->prec == PREC_X3) {
            err = launch_conv_stem_x3(d_in, batch, e->hdr.in_c, e->hdr.in_h, e->hdr.in_w, o.kh, o.pad, o.act, wb + op.w_off, (const float*)(wb + op.b_off), cv, st);
        } else if (op.fuse_conv2 >= 0) {
            const EngOp& c2 = e->ops[op.fuse_conv2];
            err = launch_conv_stem2(d_in, batch, e->hdr.in_c, e->hdr.in_h, e->hdr.in_w, o.kh, o.pad, wb + op.w_off, (const float*)(wb + op.b_off), cv,
                                    wb + c2.w_off, (const float*)(wb + c2.b_off), make_view(e, c2.f.out_buf, c2.f.out_coff, c2.f.out_c), packed_in, e->prec, st);
        } else
            err = launch_conv_stem(d_in, batch, e->hdr.in_c, e->hdr.in_h, e->hdr.in_w, o.kh, o.pad, o.act, wb + op.w_off,
                                   (const float*)(wb + op.b_off), cv, op.fuse_pool >= 0, pv, packed_in, e->prec, st);
        if (err != hipSuccess) {
            set_error("layer %d (%s): stem launch failed: %s", i, op.name.c_str(), hipGetErrorString(err));
            (void)hipGetLastError();
            return ADAS_ERR_HIP;
        }
        return ADAS_OK;
    }
    switch (o.type) {
        case OP_INPUT:
            err = launch_input_nchw(d_in, make_view(e, o.out_buf, 0, 8), batch, e->hdr.in_c, e->prec, st);
            break;
        case OP_CONV: {
            if (op.ds_user >= 0 && ds_folded(e, op.ds_user, batch)) break;   // computed inside the conv it is the shortcut of
            if (op.c2f[0] >= 0) {   // this 1x1 conv, the Bottleneck pair behind it and the block's closing 1x1 conv: one launch
                const EngOp &ca = e->ops[op.c2f[0]], &cb = e->ops[op.c2f[1]], &c2 = e->ops[op.c2f[2]];
                if (e->prec == PREC_X3) {
                    const void* const w4[4] = {wb + op.w_off, wb + ca.w_off, wb + cb.w_off, wb + c2.w_off};
                    const float* const b4[4] = {(const float*)(wb + op.b_off), (const float*)(wb + ca.b_off), (const float*)(wb + cb.b_off), (const float*)(wb + c2.b_off)};
                    err = launch_conv_c2f16_x3(make_view(e, o.in_buf[0], o.in_coff[0], o.in_c[0]), make_view(e, c2.f.out_buf, c2.f.out_coff, c2.f.out_c), w4, b4, batch, st);
                    break;
                }
                err = launch_conv_c2f16(make_view(e, o.in_buf[0], o.in_coff[0], o.in_c[0]), make_view(e, c2.f.out_buf, c2.f.out_coff, c2.f.out_c),
                                        wb + op.w_off, (const float*)(wb + op.b_off), wb + ca.w_off, (const float*)(wb + ca.b_off), wb + cb.w_off,
                                        (const float*)(wb + cb.b_off), wb + c2.w_off, (const float*)(wb + c2.b_off), batch, e->prec, st);
                break;
            }
            if (op.pair_b >= 0) {   // this conv and the one behind it, one launch
                const EngOp& b = e->ops[op.pair_b];
                err = launch_conv_pair(make_view(e, o.in_buf[0], o.in_coff[0], o.in_c[0]), make_view(e, b.f.out_buf, b.f.out_coff, b.f.out_c),
                                       wb + op.w_off, (const float*)(wb + op.b_off), wb + b.w_off, (const float*)(wb + b.b_off), batch,
                                       b.f.res_mode != RES_NONE, e->prec, st);
                break;
            }
            ConvArgs a = conv_args_of(e, i, batch);
            fold_ds(e, i, &a);
            err = launch_conv(a, st);
            break;
        }
        case OP_MAXPOOL:
            if (op.pool3[0] >= 0) {
                const FileOp &q1 = e->ops[op.pool3[0]].f, &q2 = e->ops[op.pool3[1]].f;
                const TView outs[3] = {make_view(e, o.out_buf, o.out_coff, o.out_c), make_view(e, q1.out_buf, q1.out_coff, q1.out_c),
                                       make_view(e, q2.out_buf, q2.out_coff, q2.out_c)};
                err = launch_sppf_pool3(make_view(e, o.in_buf[0], o.in_coff[0], o.in_c[0]), outs, batch, e->prec, st);
                break;
            }
            err = launch_maxpool(make_view(e, o.in_buf[0], o.in_coff[0], o.in_c[0]), make_view(e, o.out_buf, o.out_coff, o.out_c), batch,
                                 o.kh, o.stride, o.pad, e->prec, st);
            break;
        case OP_AVGPOOL:
            err = launch_avgpool(make_view(e, o.in_buf[0], o.in_coff[0], o.in_c[0]), make_view(e, o.out_buf, o.out_coff, o.out_c), batch, o.kh, o.stride,
                                 o.pad, e->prec, st);
            break;
        case OP_DEPTH2SPACE:
            err = launch_depth2space(make_view(e, o.in_buf[0], o.in_coff[0], o.in_c[0]), make_view(e, o.out_buf, o.out_coff, o.out_c), batch, e->prec, st);
            break;
        case OP_DETECT_V6: {
            TView ins[6];
            for (int k = 0; k < 6; ++k) ins[k] = make_view(e, o.in_buf[k], o.in_coff[k], o.in_c[k]);
            int strides[3] = {(int)o.params[2], (int)o.params[3], (int)o.params[4]};
            err = (o.params[5] != 0.0f ? launch_detect_v6_dfl : launch_detect_v6)(ins, (float*)e->bufs[o.out_buf].d, batch, (int)o.params[0],
                                                                                  (int)o.params[1], strides, st);
            break;
        }
        case OP_UPSAMPLE2:
            err = launch_upsample2(make_view(e, o.in_buf[0], o.in_coff[0], o.in_c[0]), make_view(e, o.out_buf, o.out_coff, o.out_c), batch,
                                   e->prec, st);
            break;
        case OP_DETECT_V8: {
            TView ins[6];
            int strides[3] = {(int)o.params[2], (int)o.params[3], (int)o.params[4]};
            if (op.det_src[0] >= 0) {  // decode + the six 1x1 convs in front of it
                const void* wf[6];
                const float* bs[6];
                for (int k = 0; k < 6; ++k) {
                    const EngOp& c = e->ops[op.det_src[k]];
                    ins[k] = make_view(e, c.f.in_buf[0], c.f.in_coff[0], c.f.in_c[0]);
                    wf[k] = wb + c.w_off;
                    bs[k] = (const float*)(wb + c.b_off);
                }
                if (e->prec == PREC_X3)
                    err = launch_detect_v8_fused_x3(ins, wf, bs, e->ops[op.det_src[0]].kpad / 32, e->ops[op.det_src[1]].kpad / 32, (float*)e->bufs[o.out_buf].d, batch,
                                                    (int)o.params[0], (int)o.params[1], strides, st, e->sink_conf, e->sink_cls);
                else
                    err = launch_detect_v8_fused(ins, wf, bs, (float*)e->bufs[o.out_buf].d, batch, (int)o.params[0], (int)o.params[1], strides, e->prec, st, e->sink_conf, e->sink_cls);
                break;
            }
            for (int k = 0; k < 6; ++k) ins[k] = make_view(e, o.in_buf[k], o.in_coff[k], o.in_c[k]);
            err = launch_detect_v8(ins, (float*)e->bufs[o.out_buf].d, batch, (int)o.params[0], (int)o.params[1], strides, st);
            break;
        }
        case OP_DETECT_V5: {
            TView ins[3];
            int strides[3] = {(int)o.params[2], (int)o.params[3], (int)o.params[4]};
            if (op.det_src[0] >= 0) {  // decode + the three 1x1 convs in front of it
                const void* wf[3];
                const float* bs[3];
                for (int k = 0; k < 3; ++k) {
                    const EngOp& c = e->ops[op.det_src[k]];
                    ins[k] = make_view(e, c.f.in_buf[0], c.f.in_coff[0], c.f.in_c[0]);
                    wf[k] = wb + c.w_off;
                    bs[k] = (const float*)(wb + c.b_off);
                }
                err = launch_detect_v5_fused(ins, wf, bs, (float*)e->bufs[o.out_buf].d, batch, (int)o.params[0], (int)o.params[1], strides,
                                             (const float*)(wb + op.w_off), e->prec, st, e->sink_conf, e->sink_cls);
                break;
            }
            for (int k = 0; k < 3; ++k) ins[k] = make_view(e, o.in_buf[k], o.in_coff[k], o.in_c[k]);
            err = launch_detect_v5(ins, (float*)e->bufs[o.out_buf].d, batch, (int)o.params[0], (int)o.params[1], strides,
                                   (const float*)(wb + op.w_off), st);
            break;
        }
        case OP_DWCONV: {
            TView r{};
            if (o.res_mode != RES_NONE) r = make_view(e, o.res_buf, o.res_coff, o.out_c);
            err = launch_dwconv(make_view(e, o.in_buf[0], o.in_coff[0], o.in_c[0]), make_view(e, o.out_buf, o.out_coff, o.out_c), r, (int)o.res_mode,
                                (const float*)(wb + op.w_off), (const float*)(wb + op.b_off), batch, (int)o.kh, (int)o.stride, (int)o.pad, (int)o.act,
                                e->prec, st);
            break;
        }
        case OP_SE_GATE: {
            const float* w1 = (const float*)(wb + op.w_off);
            const float* w2 = (const float*)(wb + op.b_off);
            TView scratch{};
            const bool has_scratch = o.res_buf >= 0 && o.res_buf < (int32_t)e->bufs.size();   // res_buf: the per-frame scratch of the two-launch form
            if (has_scratch) scratch = make_view(e, o.res_buf, 0, e->bufs[o.res_buf].c);
            err = launch_se_gate(make_view(e, o.in_buf[0], o.in_coff[0], o.in_c[0]), make_view(e, o.out_buf, o.out_coff, o.out_c), w1, w2, (int)o.params[0],
                                 (int)o.params[1], (int)o.params[2], batch, e->prec, st, has_scratch ? &scratch : nullptr);
            break;
        }
        case OP_SCALE:
            err = launch_scale(make_view(e, o.in_buf[0], o.in_coff[0], o.in_c[0]), make_view(e, o.in_buf[1], o.in_coff[1], o.in_c[1]),
                               make_view(e, o.out_buf, o.out_coff, o.out_c), batch, e->prec, st);
            break;
        case OP_SHUFFLE:
            err = launch_shuffle(make_view(e, o.in_buf[0], o.in_coff[0], o.in_c[0]), make_view(e, o.out_buf, o.out_coff, o.out_c), (int)o.params[0], batch, e->prec, st);
            break;
        case OP_WSUM: {
            TView ins[3];
            for (uint32_t k = 0; k < o.n_in && k < 3; ++k) ins[k] = make_view(e, o.in_buf[k], o.in_coff[k], o.in_c[k]);
            err = launch_wsum((int)o.n_in, ins, o.params, make_view(e, o.out_buf, o.out_coff, o.out_c), batch, (int)o.act, e->prec, st);
            break;
        }
        case OP_ATTENTION:
            err = launch_attention(make_view(e, o.in_buf[0], o.in_coff[0], o.in_c[0]), make_view(e, o.out_buf, o.out_coff, o.out_c), batch,
                                   (int)o.params[0], (int)o.params[1], (int)o.params[2], o.params[3], e->prec, st);
            break;
        case OP_LAYERNORM: {
            const EngBuf& ib = e->bufs[o.in_buf[0]];
            int len = ib.h * ib.w * ib.c;
            if (!ib.f32) { set_error("layernorm input must be fp32"); return ADAS_ERR_FORMAT; }
            err = launch_layernorm((const float*)ib.d, e->bufs[o.out_buf].d, (const float*)(wb + op.w_off), (const float*)(wb + op.b_off),
                                   batch, len, o.params[0], e->prec, st);
            break;
        }
        default:
            set_error("unknown op type %u in layer %d (%s)", o.type, i, op.name.c_str());
            return ADAS_ERR_FORMAT;
    }
    if (err != hipSuccess) {
        set_error("layer %d (%s): launch failed: %s", i, op.name.c_str(), hipGetErrorString(err));
        (void)hipGetLastError();
        return ADAS_ERR_HIP;
    }
    return ADAS_OK;
}

// Builds the multi-layer launches of this batch size (device tables: allocations and copies, so never inside a stream capture --
// adas_pipeline_* prepares before it captures; a forward that finds nothing prepared while capturing runs per-layer launches).
static void prepare_groups(adas_engine* e, int batch) {
    std::vector<GroupRun>& runs = e->groups[batch];
    const int n = (int)e->ops.size();
    int i = 0;
    while (i < n) {
        std::vector<ConvArgs> layers;
        std::vector<int> ops;
        int j = i, last = i;
        for (; j < n; ++j) {
            if (e->ops[j].skip) continue;
            if (e->ops[j].f.type == OP_CONV && e->ops[j].ds_user >= 0 && ds_folded(e, e->ops[j].ds_user, batch)) continue;
            ConvArgs a;
            if (!group_candidate(e, j, batch, &a) || (int)layers.size() >= ML_MAX_LAYERS) break;
            layers.push_back(a); ops.push_back(j);
            last = j;
        }
        if (layers.size() < 2) { i = (layers.empty() ? j : last) + 1; continue; }
        const std::vector<int> level = ml_levels(layers);
        int nlev = 0;
        for (int v : level) nlev = v + 1 > nlev ? v + 1 : nlev;
        GroupRun run;
        run.first = ops.front(); run.last = last; run.ops = ops;
        bool any_group = false, ok = true;
        for (int lv = 0; lv < nlev && ok; ++lv) {
            std::vector<int> idx;
            for (size_t k = 0; k < layers.size(); ++k)
                if (level[k] == lv) idx.push_back((int)k);
            for (size_t c0 = 0; c0 < idx.size() && ok; c0 += ML_GROUP_MAX) {   // at most ML_GROUP_MAX layers per launch
                const size_t c1 = c0 + ML_GROUP_MAX < idx.size() ? c0 + ML_GROUP_MAX : idx.size();
                GroupStep st;
                if (c1 - c0 >= 2) {
                    std::vector<ConvArgs> sub;
                    for (size_t k = c0; k < c1; ++k) { sub.push_back(layers[idx[k]]); st.members.push_back(ops[idx[k]]); }
                    std::string why;
                    st.group = ml_group_create(sub, e->prec, &why);
                    ok = st.group != nullptr;
                    any_group = true;
                } else {
                    st.op = ops[idx[c0]];
                    st.members.push_back(st.op);
                }
                if (ok) run.steps.push_back(st);
            }
        }
        if (ok && any_group) runs.push_back(run);
        else
            for (auto& st : run.steps) ml_group_destroy(st.group);
        i = last + 1;
    }
}

// Tables are kept for the life of the engine (a captured hipGraph may reference them): at most this many distinct batch sizes get
// them, later ones run one launch per layer.
constexpr size_t kMaxPreparedBatches = 16;

// The allocations and copies below must not land in -- or invalidate -- a stream capture the calling thread has open on ANOTHER stream
// (engine_forward only knows its own): they run with the thread's capture mode relaxed, restored on every exit.
struct RelaxedCaptureMode {
    hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
    bool ok;
    RelaxedCaptureMode() { ok = hipThreadExchangeStreamCaptureMode(&mode) == hipSuccess; if (!ok) (void)hipGetLastError(); }
    ~RelaxedCaptureMode() { if (ok && hipThreadExchangeStreamCaptureMode(&mode) != hipSuccess) (void)hipGetLastError(); }
};

int engine_prepare(adas_engine* e, int batch) {
    const bool want_groups = e->group_on && !e->groups.count(batch), want_ml = ml_enabled(e) && !e->ml.count(batch);
    if (!want_groups && !want_ml) return ADAS_OK;
    RelaxedCaptureMode relaxed;
    if (want_groups) {
        if (e->groups.size() >= kMaxPreparedBatches) e->groups[batch];   // an empty list: per-layer launches for this batch size
        else prepare_groups(e, batch);
    }
    if (!want_ml) return ADAS_OK;
    if (e->ml.size() >= kMaxPreparedBatches) { e->ml[batch]; return ADAS_OK; }
    std::vector<MlSeg>& segs = e->ml[batch];
    static int min_layers = -1, max_items = -1;
    if (min_layers < 0) { const char* v = getenv("ADAS_ML_MIN_LAYERS"); min_layers = v ? atoi(v) : 2; if (min_layers < 1) min_layers = 1; }
    if (max_items < 0) { const char* v = getenv("ADAS_ML_MAX_LAYER_ITEMS"); max_items = v ? atoi(v) : 0; }   // experiments: keep layers with more items out
    const int n = (int)e->ops.size();
    int i = 0;
    while (i < n) {
        std::vector<ConvArgs> layers;
        std::vector<int> kernels, ops;
        int j = i, last = i;
        for (; j < n; ++j) {
            if (e->ops[j].skip) continue;            // launches nothing (fused into a neighbour): transparent
            if (e->ops[j].f.type == OP_CONV && e->ops[j].ds_user >= 0 && ds_folded(e, e->ops[j].ds_user, batch)) continue;
            ConvArgs a;
            if (!ml_candidate(e, j, batch, &a) || (int)layers.size() >= ML_MAX_LAYERS) break;
            if (max_items > 0) {
                const long wgs = (long)((a.m + 255) / 256) * ((a.out.c + 63) / 64);
                if (wgs > max_items) break;
            }
            layers.push_back(a); kernels.push_back(e->ops[j].kernel); ops.push_back(j);
            last = j;
        }
        if ((int)layers.size() >= min_layers) {
            std::string why;
            MlPlanInfo info;
            MlPlan* pl = ml_plan_create(layers, kernels, e->prec, &why, &info);
            if (pl) {
                MlSeg sg;
                sg.first = ops.front(); sg.last = last; sg.n_layers = (int)layers.size(); sg.n_items = info.n_items; sg.plan = pl; sg.ops = ops;
                segs.push_back(sg);
            }
            i = last + 1;
        } else {
            i = (layers.empty() ? j : last) + 1;
        }
    }
    return ADAS_OK;
}

static bool stream_capturing(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return false; }
    return cs != hipStreamCaptureStatusNone;
}

int engine_forward(adas_engine* e, const float* d_in, int batch, hipStream_t st, bool packed_in) {
    if (((ml_enabled(e) && !e->ml.count(batch)) || (e->group_on && !e->groups.count(batch))) && !stream_capturing(st)) {
        int rc = engine_prepare(e, batch);
        if (rc != ADAS_OK) return rc;
    }
    const std::vector<MlSeg>* segs = ml_segments(e, batch);
    const std::vector<GroupRun>* runs = group_runs(e, batch);
    size_t si = 0, gi = 0;
    for (int i = 0; i < (int)e->ops.size(); ++i) {
        if (runs && gi < runs->size() && (*runs)[gi].first == i) {   // a run of halo convs, level by level: independent layers share a launch
            const GroupRun& run = (*runs)[gi++];
            for (auto& step : run.steps) {
                if (step.group) {
                    hipError_t err = ml_group_launch(step.group, st);
                    if (err != hipSuccess) {
                        set_error("layers %d..%d: grouped launch failed: %s", run.first, run.last, hipGetErrorString(err));
                        (void)hipGetLastError();
                        return ADAS_ERR_HIP;
                    }
                } else {
                    int rc = engine_run_op(e, step.op, d_in, batch, st, packed_in);
                    if (rc != ADAS_OK) return rc;
                }
            }
            i = run.last;
            continue;
        }
        if (segs && si < segs->size() && (*segs)[si].first == i) {
            const MlSeg& sg = (*segs)[si++];
            hipError_t err = ml_launch(sg.plan, st);
            if (err != hipSuccess) {
                set_error("layers %d..%d (%s ...): multi-layer launch failed: %s", sg.first, sg.last, e->ops[sg.first].name.c_str(), hipGetErrorString(err));
                (void)hipGetLastError();
                return ADAS_ERR_HIP;
            }
            i = sg.last;
            continue;
        }
        int rc = engine_run_op(e, i, d_in, batch, st, packed_in);
        if (rc != ADAS_OK) return rc;
    }
    return ADAS_OK;
}
}  // namespace adas

extern "C" {

int adas_engine_infer_device(adas_engine* e, const float* d_input, int batch, void* stream) {
    ADAS_REQUIRE(e && d_input && batch > 0 && batch <= e->max_batch, ADAS_ERR_INVALID, "adas_engine_infer_device: bad argument (batch %d, max %d)", batch,
                 e ? e->max_batch : 0);
    e->last = (hipStream_t)stream;
    return engine_forward(e, d_input, batch, (hipStream_t)stream);
}

int adas_engine_prepare(adas_engine* e, int batch) {
    ADAS_REQUIRE(e && batch > 0 && batch <= e->max_batch, ADAS_ERR_INVALID, "adas_engine_prepare: bad argument (batch %d, max %d)", batch, e ? e->max_batch : 0);
    return engine_prepare(e, batch);
}
int adas_engine_ml_info(const adas_engine* e, int batch, int32_t* n_launches, int32_t* n_layers, int32_t* n_items) {
    ADAS_REQUIRE(e && batch > 0, ADAS_ERR_INVALID, "adas_engine_ml_info: bad argument");
    int nl = 0, ni = 0, ns = 0;
    if (const std::vector<MlSeg>* segs = ml_segments(e, batch))
        for (auto& sg : *segs) { ++ns; nl += sg.n_layers; ni += sg.n_items; }
    if (n_launches) *n_launches = ns;
    if (n_layers) *n_layers = nl;
    if (n_items) *n_items = ni;
    return ADAS_OK;
}
int adas_engine_ml_status(const adas_engine* e, int batch, uint32_t* error_word) {
    ADAS_REQUIRE(e && error_word, ADAS_ERR_INVALID, "adas_engine_ml_status: bad argument");
    *error_word = 0;
    if (const std::vector<MlSeg>* segs = ml_segments(e, batch))
        for (auto& sg : *segs) {
            unsigned w = 0;
            ADAS_REQUIRE(ml_plan_status(sg.plan, &w) == 0, ADAS_ERR_HIP, "adas_engine_ml_status: could not read the control block");
            if (w) {
                *error_word = w;
                set_error("multi-layer launch of layers %d..%d: a dependency wait timed out (item %u)", sg.first, sg.last, w - 1);
                return ADAS_ERR_HIP;
            }
        }
    return ADAS_OK;
}
int adas_engine_ml_counters(const adas_engine* e, int batch, int launch, uint32_t head16[16]) {
    ADAS_REQUIRE(e && head16, ADAS_ERR_INVALID, "adas_engine_ml_counters: bad argument");
    const std::vector<MlSeg>* segs = ml_segments(e, batch);
    ADAS_REQUIRE(segs && launch >= 0 && launch < (int)segs->size(), ADAS_ERR_INVALID, "adas_engine_ml_counters: no multi-layer launch %d at batch %d", launch, batch);
    unsigned w = 0;
    ADAS_REQUIRE(ml_plan_status((*segs)[launch].plan, &w, head16) == 0, ADAS_ERR_HIP, "adas_engine_ml_counters: could not read the control block");
    return ADAS_OK;
}
int adas_engine_launch_count(adas_engine* e, int batch) {
    if (!e || batch <= 0 || batch > e->max_batch) return -1;
    const std::vector<MlSeg>* segs = ml_segments(e, batch);
    const std::vector<GroupRun>* runs = group_runs(e, batch);
    size_t si = 0, gi = 0;
    int n = 0;
    for (int i = 0; i < (int)e->ops.size(); ++i) {
        if (runs && gi < runs->size() && (*runs)[gi].first == i) { n += (int)(*runs)[gi].steps.size(); i = (*runs)[gi++].last; continue; }
        if (segs && si < segs->size() && (*segs)[si].first == i) { ++n; i = (*segs)[si++].last; continue; }
        const EngOp& op = e->ops[i];
        if (op.skip) continue;
        if (op.f.type == OP_CONV && op.ds_user >= 0 && ds_folded(e, op.ds_user, batch)) continue;
        ++n;
    }
    return n;
}

// The ConvArgs a layer description stands for at this batch (no device: the pointers are placeholders that are never read).
static ConvArgs conv_args_of_desc(const adas_ml_layer_desc& d, int batch, int precision) {
    auto view = [](const adas_ml_view& v) {
        TView t;
        t.p = (void*)(uintptr_t)v.buf; t.cs = v.cs; t.coff = v.coff; t.c = v.c; t.h = v.h; t.w = v.w; t.f32 = 0;
        return t;
    };
    ConvArgs a;
    a.in = view(d.x); a.out = view(d.y);
    if (d.res_mode != RES_NONE) a.res = view(d.res);
    else { a.res = a.out; a.res.p = nullptr; }
    a.wgt = (const void*)(uintptr_t)0x1000; a.bias = (const float*)(uintptr_t)0x1000;
    a.n = batch; a.kh = a.kw = d.kernel == CONV_PW ? 1 : 3; a.stride = d.stride; a.pad = d.kernel == CONV_PW ? 0 : 1; a.act = d.act; a.res_mode = d.res_mode;
    a.k = a.kh * a.kw * a.in.c; a.kpad = (a.kh * a.kw * ((a.in.c + 31) / 32 * 32) + 31) / 32 * 32; a.m = batch * a.out.h * a.out.w; a.max_n = batch; a.prec = precision;
    a.halo_bn = d.halo_bn;
    if (d.up_c > 0) { a.up = view(d.up); a.up_c = d.up_c; }
    return a;
}

int adas_debug_ml_plan(const adas_ml_layer_desc* layers, int n_layers, int batch, int precision, int32_t* deps, int32_t* targets, uint64_t* items,
                       int items_cap, int32_t summary[4]) {
    ADAS_REQUIRE(layers && n_layers > 0 && batch > 0 && deps && targets && summary, ADAS_ERR_INVALID, "adas_debug_ml_plan: bad argument");
    std::vector<ConvArgs> ls;
    std::vector<int> ks;
    for (int i = 0; i < n_layers; ++i) {
        ls.push_back(conv_args_of_desc(layers[i], batch, precision));
        ks.push_back(layers[i].kernel);
    }
    std::string why;
    MlPlanInfo info;
    MlPlan* pl = ml_plan_create(ls, ks, precision, &why, &info, true);
    ADAS_REQUIRE(pl, ADAS_ERR_INVALID, "adas_debug_ml_plan: %s", why.c_str());
    ml_plan_destroy(pl);
    for (int i = 0; i < n_layers; ++i)
        for (int k = 0; k < ML_MAX_DEPS; ++k) {
            deps[i * ML_MAX_DEPS + k] = k < (int)info.deps[i].size() ? info.deps[i][k] : -1;
            targets[i * ML_MAX_DEPS + k] = k < (int)info.targets[i].size() ? info.targets[i][k] : 0;
        }
    summary[0] = info.n_items; summary[1] = info.grid; summary[2] = (int32_t)info.lds; summary[3] = info.order;
    if (items) {
        ADAS_REQUIRE(items_cap >= info.n_items, ADAS_ERR_CAPACITY, "adas_debug_ml_plan: %d items, room for %d", info.n_items, items_cap);
        for (int k = 0; k < info.n_items; ++k) items[k] = info.item_words[k];
    }
    return ADAS_OK;
}

int adas_debug_conv_route(const adas_ml_layer_desc* layer, int batch, int precision, char* name, int name_cap) {
    ADAS_REQUIRE(layer && batch > 0 && precision >= PREC_BF16 && precision <= PREC_X3 && name && name_cap > 0, ADAS_ERR_INVALID,
                 "adas_debug_conv_route: bad argument");
    ConvArgs a = conv_args_of_desc(*layer, batch, precision);
    const ConvPlan pl = plan_conv(precision, a.kh, a.kw, a.stride, a.pad, a.max_n, a.res_mode, a.in, a.out);
    a.kpad = pl.kpad;
    // the second weight packing of the split precision, where the engine would allocate it when it loads the layer
    if (wants_x3h8_packing(precision, pl.kernel, a.kh, a.kw, a.stride, a.pad, a.res_mode, a.in, a.out)) a.wgt_h8x3 = (const void*)(uintptr_t)0x1000;
    snprintf(name, name_cap, "%s", conv_kernel_name(a));
    return ADAS_OK;
}

int adas_engine_precision(const adas_engine* e) { return e ? e->prec : -1; }
int adas_engine_model_io_half(const adas_engine* e) { return e ? (int)((e->hdr.in_cpad >> 16) & 1u) : 0; }

int adas_engine_accepts_packed_input(const adas_engine* e) {
    // (the split precision's stem reads the fp32 seam tensor: a 16-bit packed pixel could not carry its 22 bits)
    return (e && e->prec != PREC_X3 && e->ops.size() >= 2 && e->ops[0].skip && e->ops[1].kernel == CONV_STEM) ? 1 : 0;
}

int adas_engine_infer_device_packed(adas_engine* e, const uint16_t* d_input_nhwc4, int batch, void* stream) {
    ADAS_REQUIRE(e && d_input_nhwc4 && batch > 0 && batch <= e->max_batch, ADAS_ERR_INVALID, "adas_engine_infer_device_packed: bad argument");
    ADAS_REQUIRE(adas_engine_accepts_packed_input(e), ADAS_ERR_INVALID,
                 "this engine's first layer is not the fused stem (fp32 mode or ADAS_NO_STEM): feed the fp32 NCHW tensor instead");
    e->last = (hipStream_t)stream;
    return engine_forward(e, reinterpret_cast<const float*>(d_input_nhwc4), batch, (hipStream_t)stream, true);
}

const float* adas_engine_output_device(const adas_engine* e, int index) {
    if (!e || index < 0 || index >= (int)e->outs.size()) return nullptr;
    const EngOut& o = e->outs[index];
    return (const float*)e->bufs[o.buf].d + o.offset;
}

int adas_engine_infer_host(adas_engine* e, const float* h_input, int batch, float* const* h_outputs) {
    ADAS_REQUIRE(e && h_input && h_outputs && batch > 0 && batch <= e->max_batch, ADAS_ERR_INVALID, "adas_engine_infer_host: bad argument");
    size_t in_bytes = (size_t)batch * e->hdr.in_c * e->hdr.in_h * e->hdr.in_w * 4;
    ADAS_HIP_TRY(hipMemcpyAsync(e->d_input, h_input, in_bytes, hipMemcpyHostToDevice, 0));
    int rc = adas_engine_infer_device(e, e->d_input, batch, nullptr);
    if (rc != ADAS_OK) return rc;
    for (size_t i = 0; i < e->outs.size(); ++i) {
        const EngOut& o = e->outs[i];
        const EngBuf& b = e->bufs[o.buf];
        size_t frame_stride = (size_t)b.h * b.w * b.c;  // floats per frame in the backing buffer
        ADAS_HIP_TRY(hipMemcpy2DAsync(h_outputs[i], o.elems * 4, (const float*)b.d + o.offset, frame_stride * 4, o.elems * 4, batch,
                                      hipMemcpyDeviceToHost, 0));
    }
    ADAS_HIP_TRY(hipStreamSynchronize(0));
    // opt-in multi-layer launches (ADAS_ML=1): a dependency wait that timed out leaves its item uncomputed -- the caller gets an error,
    // never the partial outputs
    if (ml_enabled(e)) {
        uint32_t w = 0;
        int rc = adas_engine_ml_status(e, batch, &w);
        if (rc != ADAS_OK) return rc;
    }
    return ADAS_OK;
}

int adas_engine_profile(adas_engine* e, const float* d_input, int batch, int iters, float* ms_per_layer, int max_layers, int* num_layers) {
    ADAS_REQUIRE(e && d_input && batch > 0 && batch <= e->max_batch && iters > 0 && ms_per_layer, ADAS_ERR_INVALID, "adas_engine_profile: bad argument");
    const int n = (int)e->ops.size();
    ADAS_REQUIRE(max_layers >= n, ADAS_ERR_INVALID, "need room for %d layers", n);
    if ((int)e->events.size() < n + 1) {
        e->events.resize(n + 1, nullptr);
        for (auto& ev : e->events)
            if (!ev) ADAS_HIP_TRY(hipEventCreate(&ev));
    }
    for (int i = 0; i < n; ++i) ms_per_layer[i] = 0.f;
    // an event record is itself a packet on the stream (~5 us between two records with nothing in between): measured here and taken
    // off every layer, so that a layer that launches nothing (fused / folded into a neighbour) reads 0 and the per-layer sum is the
    // kernels' time, not kernels + markers
    float marker_ms = 0.f;
    {
        const int reps = n < 8 ? n : 8;
        for (int r = 0; r <= reps; ++r) ADAS_HIP_TRY(hipEventRecord(e->events[r], 0));
        ADAS_HIP_TRY(hipStreamSynchronize(0));
        float lo = 1e30f;
        for (int r = 1; r < reps; ++r) {   // (the first gap carries the stream's wake-up)
            float ms = 0.f;
            ADAS_HIP_TRY(hipEventElapsedTime(&ms, e->events[r], e->events[r + 1]));
            lo = ms < lo ? ms : lo;
        }
        marker_ms = lo < 1e29f ? lo : 0.f;
    }
    {
        int rc = engine_prepare(e, batch);
        if (rc != ADAS_OK) return rc;
    }
    const std::vector<MlSeg>* segs = ml_segments(e, batch);
    const std::vector<GroupRun>* runs = group_runs(e, batch);
    struct StepMark { int layer, ev, prev; };   // prev: index into step_events, or -(layer index + 1) of the layer event that opens the run
    for (int it = 0; it < iters; ++it) {
        ADAS_HIP_TRY(hipEventRecord(e->events[0], 0));
        size_t si = 0, gi = 0, n_step_ev = 0;
        std::vector<StepMark> step_marks;
        for (int i = 0; i < n; ++i) {
            if (runs && gi < runs->size() && (*runs)[gi].first == i) {
                // a run of halo convs, launched level by level: one event per STEP, a step's time goes to its first member (the layer
                // adas_engine_layer_kernel labels with the step's kernel), every other layer of the run reads 0
                const GroupRun& run = (*runs)[gi++];
                const size_t base = step_marks.size();
                for (auto& step : run.steps) {
                    if (step.group) {
                        hipError_t err = ml_group_launch(step.group, 0);
                        if (err != hipSuccess) return hip_fail(err, "grouped launch", __FILE__, __LINE__);
                    } else {
                        int rc = engine_run_op(e, step.op, d_input, batch, 0);
                        if (rc != ADAS_OK) return rc;
                    }
                    if (n_step_ev >= e->step_events.size()) {
                        hipEvent_t ev = nullptr;
                        ADAS_HIP_TRY(hipEventCreate(&ev));
                        e->step_events.push_back(ev);
                    }
                    ADAS_HIP_TRY(hipEventRecord(e->step_events[n_step_ev], 0));
                    step_marks.push_back({step.members.front(), (int)n_step_ev, step_marks.size() == base ? -(i + 1) : (int)n_step_ev - 1});
                    ++n_step_ev;
                }
                for (int k = i; k <= run.last; ++k) ADAS_HIP_TRY(hipEventRecord(e->events[k + 1], 0));
                i = run.last;
                continue;
            }
            if (segs && si < segs->size() && (*segs)[si].first == i) {   // a multi-layer launch: its time goes to its first layer, the rest read 0
                const MlSeg& sg = (*segs)[si++];
                hipError_t err = ml_launch(sg.plan, 0);
                if (err != hipSuccess) return hip_fail(err, "multi-layer launch", __FILE__, __LINE__);
                for (int k = i; k <= sg.last; ++k) ADAS_HIP_TRY(hipEventRecord(e->events[k + 1], 0));
                i = sg.last;
                continue;
            }
            int rc = engine_run_op(e, i, d_input, batch, 0);
            if (rc != ADAS_OK) return rc;
            ADAS_HIP_TRY(hipEventRecord(e->events[i + 1], 0));
        }
        ADAS_HIP_TRY(hipStreamSynchronize(0));
        std::vector<char> in_run(n, 0);
        if (runs)
            for (auto& run : *runs)
                for (int k = run.first; k <= run.last; ++k) in_run[k] = 1;
        for (int i = 0; i < n; ++i) {
            if (in_run[i]) continue;          // layers of a grouped run are timed per step below
            float ms = 0.f;
            ADAS_HIP_TRY(hipEventElapsedTime(&ms, e->events[i], e->events[i + 1]));
            ms -= marker_ms;
            ms_per_layer[i] += (ms > 0.f ? ms : 0.f) / (float)iters;
        }
        for (auto& mk : step_marks) {
            float ms = 0.f;
            hipEvent_t from = mk.prev < 0 ? e->events[-mk.prev - 1] : e->step_events[mk.prev];
            ADAS_HIP_TRY(hipEventElapsedTime(&ms, from, e->step_events[mk.ev]));
            ms -= marker_ms;
            ms_per_layer[mk.layer] += (ms > 0.f ? ms : 0.f) / (float)iters;
        }
    }
    if (num_layers) *num_layers = n;
    return ADAS_OK;
}

int adas_engine_fetch_activation(adas_engine* e, int layer, int batch, float* h_out, int64_t dims[4]) {
    ADAS_REQUIRE(e && layer >= 0 && layer < (int)e->ops.size() && batch > 0 && batch <= e->max_batch, ADAS_ERR_INVALID, "bad layer/batch");
    const FileOp& o = e->ops[layer].f;
    ADAS_REQUIRE(!(e->ops[layer].skip && o.type == OP_CONV && (e->ops[layer].kernel == CONV_PW || e->ops[layer].kernel == CONV_DET5)), ADAS_ERR_INVALID,
                 "layer %d (%s) is fused into the Detect launch and has no materialised activation (ADAS_NO_DETECT_FUSE=1 keeps it)", layer,
                 e->ops[layer].name.c_str());
    ADAS_REQUIRE(!(e->ops[layer].skip && o.type == OP_INPUT) &&
                     !(e->ops[layer].kernel == CONV_STEM && (e->ops[layer].fuse_pool >= 0 || e->ops[layer].fuse_conv2 >= 0)), ADAS_ERR_INVALID,
                 "layer %d (%s) is fused into the stem launch and has no materialised activation (ADAS_NO_STEM=1 keeps it)", layer,
                 e->ops[layer].name.c_str());
    ADAS_REQUIRE(!(e->ops[layer].ds_user >= 0 && ds_folded(e, e->ops[layer].ds_user, batch)), ADAS_ERR_INVALID,
                 "layer %d (%s) is a projection shortcut computed inside the conv that adds it at this batch (ADAS_NO_DS_FUSE=1 keeps it)", layer,
                 e->ops[layer].name.c_str());
    ADAS_REQUIRE(!(e->ops[layer].skip && o.type == OP_UPSAMPLE2), ADAS_ERR_INVALID,
                 "layer %d (%s) is folded into its consumer's loads and has no materialised activation (ADAS_NO_UPSAMPLE_FOLD=1 keeps it)", layer,
                 e->ops[layer].name.c_str());
    {   // a fused C2f launch materialises only its cv2 output: cv1 and the Bottleneck's two convs stay in LDS
        const bool c2f_hidden = e->ops[layer].c2f[0] >= 0 || (in_c2f(e, layer) && !is_c2f_tail(e, layer));
        ADAS_REQUIRE(!c2f_hidden, ADAS_ERR_INVALID,
                     "layer %d (%s) is computed inside a fused C2f launch: its activation stays in LDS (ADAS_NO_C2F_FUSE=1 keeps it)", layer,
                     e->ops[layer].name.c_str());
    }
    ADAS_REQUIRE(e->ops[layer].pair_b < 0, ADAS_ERR_INVALID,
                 "layer %d (%s) is the first conv of a fused 3x3 pair: its activation stays in LDS (ADAS_NO_PAIR_FUSE=1 keeps it)", layer,
                 e->ops[layer].name.c_str());
    TView v = make_view(e, o.out_buf, o.out_coff, o.out_c);
    if (o.type == OP_INPUT) v.c = 8;
    if (dims) { dims[0] = batch; dims[1] = v.c; dims[2] = v.h; dims[3] = v.w; }
    if (!h_out) return ADAS_OK;
    size_t n = (size_t)batch * v.c * v.h * v.w;
    float* d_tmp = nullptr;
    ADAS_HIP_TRY(hipMalloc((void**)&d_tmp, n * 4));
    hipError_t err = launch_nhwc_to_nchw(v, d_tmp, batch, e->prec, 0);
    if (err == hipSuccess) err = hipMemcpy(h_out, d_tmp, n * 4, hipMemcpyDeviceToHost);
    (void)hipFree(d_tmp);
    if (err != hipSuccess) return hip_fail(err, "fetch_activation", __FILE__, __LINE__);
    return ADAS_OK;
}

}  // extern "C"
