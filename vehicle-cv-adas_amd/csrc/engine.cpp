// engine.cpp -- HipEngine: runs a loaded ADASHIP1 model (engine_load.cpp: adas_engine_create) on one MI355X.
// Replaces EngineBase / OnnxEngine / TensorRTEngine (coreEngine.py:7-39,120-186): same surface
// (input shape, output shapes+names, inference on an NCHW tensor), plus a device-resident form.
#include "engine.h"
#include <string.h>
#include <string>
#include <vector>

using namespace adas;

int adas::free_engine(adas_engine* e) {
    if (!e) return ADAS_OK;
    for (auto& kv : e->schedules) free_schedule(&kv.second);
    e->schedules.clear();
    for (auto& b : e->bufs)
        if (b.d && b.alias_of < 0) (void)hipFree(b.d);
    if (e->d_weights) (void)hipFree(e->d_weights);
    if (e->d_input) (void)hipFree(e->d_input);
    for (auto& ev : e->events)
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
    Schedule local;
    layer_label(e, schedule_at(e, batch, &local), layer, batch, name, cap);
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
namespace {

const void* wgt(const adas_engine* e, const EngOp& op) { return (const unsigned char*)e->d_weights + op.w_off; }
const float* bias(const adas_engine* e, const EngOp& op) { return (const float*)((const unsigned char*)e->d_weights + op.b_off); }

// A fused Detect launch computes the n 1x1 convs in front of the decode itself (det_src): their inputs, weights and biases.
void detect_sources(const adas_engine* e, const EngOp& op, int n, TView* ins, const void** wf, const float** bs) {
    for (int k = 0; k < n; ++k) {
        const EngOp& c = e->ops[op.det_src[k]];
        ins[k] = in_view(e, c.f);
        wf[k] = wgt(e, c);
        bs[k] = bias(e, c);
    }
}

// One OP step: layer step.lead on its own kernel, with everything the schedule put into its launch.
int engine_run_op(adas_engine* e, const Step& step, const float* d_in, int batch, hipStream_t st, bool packed_in) {
    const int i = step.lead;
    const EngOp& op = e->ops[i];
    const FileOp& o = op.f;
    const int in_c = e->hdr.in_c, in_h = e->hdr.in_h, in_w = e->hdr.in_w, prec = e->prec;
    hipError_t err = hipSuccess;
    if (o.type == OP_CONV && op.kernel == CONV_STEM) {
        const TView cv = out_view(e, o);
        const TView pv = op.fuse_pool >= 0 ? out_view(e, e->ops[op.fuse_pool].f) : cv;
        if (op.fuse_conv2 >= 0) {
            const EngOp& c2 = e->ops[op.fuse_conv2];
            err = prec == PREC_X3 ? launch_conv_stem2_x3(d_in, batch, in_c, in_h, in_w, o.kh, o.pad, wgt(e, op), bias(e, op), cv, wgt(e, c2), bias(e, c2), out_view(e, c2.f), st)
                                  : launch_conv_stem2(d_in, batch, in_c, in_h, in_w, o.kh, o.pad, wgt(e, op), bias(e, op), cv, wgt(e, c2), bias(e, c2), out_view(e, c2.f),
                                                      packed_in, prec, st);
        } else if (prec == PREC_X3 && op.fuse_pool >= 0) {
            err = launch_conv_stem_pool_x3(d_in, batch, in_c, in_h, in_w, o.pad, wgt(e, op), bias(e, op), cv, pv, st);
        } else if (prec == PREC_X3) {
            err = launch_conv_stem_x3(d_in, batch, in_c, in_h, in_w, o.kh, o.pad, o.act, wgt(e, op), bias(e, op), cv, st);
        } else
            err = launch_conv_stem(d_in, batch, in_c, in_h, in_w, o.kh, o.pad, o.act, wgt(e, op), bias(e, op), cv, op.fuse_pool >= 0, pv, packed_in, prec, st);
        if (err != hipSuccess) {
            set_error("layer %d (%s): stem launch failed: %s", i, op.name.c_str(), hipGetErrorString(err));
            (void)hipGetLastError();
            return ADAS_ERR_HIP;
        }
        return ADAS_OK;
    }
    float* const head = (float*)e->bufs[o.out_buf].d;                                 // the Detect ops' output
    const int strides[3] = {(int)o.params[2], (int)o.params[3], (int)o.params[4]};    // ... and pyramid strides
    switch (o.type) {
        case OP_INPUT:
            err = launch_input_nchw(d_in, make_view(e, o.out_buf, 0, 8), batch, in_c, prec, st);
            break;
        case OP_CONV: {
            if (op.c2f[0] >= 0) {   // this 1x1 conv, the Bottleneck pair behind it and the block's closing 1x1 conv: one launch
                const EngOp &ca = e->ops[op.c2f[0]], &cb = e->ops[op.c2f[1]], &c2 = e->ops[op.c2f[2]];
                if (prec == PREC_X3) {
                    const void* const w4[4] = {wgt(e, op), wgt(e, ca), wgt(e, cb), wgt(e, c2)};
                    const float* const b4[4] = {bias(e, op), bias(e, ca), bias(e, cb), bias(e, c2)};
                    err = launch_conv_c2f16_x3(in_view(e, o), out_view(e, c2.f), w4, b4, batch, st);
                    break;
                }
                err = launch_conv_c2f16(in_view(e, o), out_view(e, c2.f), wgt(e, op), bias(e, op), wgt(e, ca), bias(e, ca), wgt(e, cb), bias(e, cb), wgt(e, c2),
                                        bias(e, c2), batch, prec, st);
                break;
            }
            if (op.pair_b >= 0) {   // this conv and the one behind it, one launch
                const EngOp& b = e->ops[op.pair_b];
                err = launch_conv_pair(in_view(e, o), out_view(e, b.f), wgt(e, op), bias(e, op), wgt(e, b), bias(e, b), batch, b.f.res_mode != RES_NONE, prec, st);
                break;
            }
            ConvArgs a = conv_args_of(e, i, batch);
            if (step.folds_shortcut) attach_shortcut(e, i, &a);
            err = launch_conv(a, st);
            break;
        }
        case OP_MAXPOOL:
            if (op.pool3[0] >= 0) {
                const TView outs[3] = {out_view(e, o), out_view(e, e->ops[op.pool3[0]].f), out_view(e, e->ops[op.pool3[1]].f)};
                err = launch_sppf_pool3(in_view(e, o), outs, batch, prec, st);
                break;
            }
            err = launch_maxpool(in_view(e, o), out_view(e, o), batch, o.kh, o.stride, o.pad, prec, st);
            break;
        case OP_AVGPOOL:
            err = launch_avgpool(in_view(e, o), out_view(e, o), batch, o.kh, o.stride, o.pad, prec, st);
            break;
        case OP_DEPTH2SPACE:
            err = launch_depth2space(in_view(e, o), out_view(e, o), batch, prec, st);
            break;
        case OP_DETECT_V6: {
            TView ins[6];
            for (int k = 0; k < 6; ++k) ins[k] = in_view(e, o, k);
            err = (o.params[5] != 0.0f ? launch_detect_v6_dfl : launch_detect_v6)(ins, head, batch, (int)o.params[0], (int)o.params[1], strides, st);
            break;
        }
        case OP_UPSAMPLE2:
            err = launch_upsample2(in_view(e, o), out_view(e, o), batch, prec, st);
            break;
        case OP_DETECT_V8: {
            TView ins[6];
            if (op.det_src[0] >= 0) {  // decode + the six 1x1 convs in front of it
                const void* wf[6];
                const float* bs[6];
                detect_sources(e, op, 6, ins, wf, bs);
                if (prec == PREC_X3)
                    err = launch_detect_v8_fused_x3(ins, wf, bs, e->ops[op.det_src[0]].kpad / 32, e->ops[op.det_src[1]].kpad / 32, head, batch, (int)o.params[0],
                                                    (int)o.params[1], strides, st, e->sink_conf, e->sink_cls);
                else
                    err = launch_detect_v8_fused(ins, wf, bs, head, batch, (int)o.params[0], (int)o.params[1], strides, prec, st, e->sink_conf, e->sink_cls);
                break;
            }
            for (int k = 0; k < 6; ++k) ins[k] = in_view(e, o, k);
            err = launch_detect_v8(ins, head, batch, (int)o.params[0], (int)o.params[1], strides, st);
            break;
        }
        case OP_DETECT_V5: {
            TView ins[3];
            if (op.det_src[0] >= 0) {  // decode + the three 1x1 convs in front of it
                const void* wf[3];
                const float* bs[3];
                detect_sources(e, op, 3, ins, wf, bs);
                err = launch_detect_v5_fused(ins, wf, bs, head, batch, (int)o.params[0], (int)o.params[1], strides, (const float*)wgt(e, op), prec, st, e->sink_conf,
                                             e->sink_cls);
                break;
            }
            for (int k = 0; k < 3; ++k) ins[k] = in_view(e, o, k);
            err = launch_detect_v5(ins, head, batch, (int)o.params[0], (int)o.params[1], strides, (const float*)wgt(e, op), st);
            break;
        }
        case OP_DWCONV: {
            TView r{};
            if (o.res_mode != RES_NONE) r = make_view(e, o.res_buf, o.res_coff, o.out_c);
            err = launch_dwconv(in_view(e, o), out_view(e, o), r, (int)o.res_mode, (const float*)wgt(e, op), bias(e, op), batch, (int)o.kh, (int)o.stride, (int)o.pad,
                                (int)o.act, prec, st);
            break;
        }
        case OP_SE_GATE: {
            TView scratch{};
            const bool has_scratch = o.res_buf >= 0 && o.res_buf < (int32_t)e->bufs.size();   // res_buf: the per-frame scratch of the two-launch form
            if (has_scratch) scratch = make_view(e, o.res_buf, 0, e->bufs[o.res_buf].c);
            err = launch_se_gate(in_view(e, o), out_view(e, o), (const float*)wgt(e, op), bias(e, op), (int)o.params[0], (int)o.params[1], (int)o.params[2], batch, prec,
                                 st, has_scratch ? &scratch : nullptr);
            break;
        }
        case OP_SCALE:
            err = launch_scale(in_view(e, o, 0), in_view(e, o, 1), out_view(e, o), batch, prec, st);
            break;
        case OP_SHUFFLE:
            err = launch_shuffle(in_view(e, o), out_view(e, o), (int)o.params[0], batch, prec, st);
            break;
        case OP_WSUM: {
            TView ins[3];
            for (uint32_t k = 0; k < o.n_in && k < 3; ++k) ins[k] = in_view(e, o, k);
            err = launch_wsum((int)o.n_in, ins, o.params, out_view(e, o), batch, (int)o.act, prec, st);
            break;
        }
        case OP_ATTENTION:
            err = launch_attention(in_view(e, o), out_view(e, o), batch, (int)o.params[0], (int)o.params[1], (int)o.params[2], o.params[3], prec, st);
            break;
        case OP_LAYERNORM: {
            const EngBuf& ib = e->bufs[o.in_buf[0]];
            int len = ib.h * ib.w * ib.c;
            if (!ib.f32) { set_error("layernorm input must be fp32"); return ADAS_ERR_FORMAT; }
            err = launch_layernorm((const float*)ib.d, e->bufs[o.out_buf].d, (const float*)wgt(e, op), bias(e, op), batch, len, o.params[0], prec, st);
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

// One step of a schedule, whatever its kind.
int run_step(adas_engine* e, const Step& step, const float* d_in, int batch, hipStream_t st, bool packed_in) {
    if (step.kind == Step::OP) return engine_run_op(e, step, d_in, batch, st, packed_in);
    const hipError_t err = step.kind == Step::GROUP ? ml_group_launch(step.group, st) : ml_launch(step.plan, st);
    if (err == hipSuccess) return ADAS_OK;
    if (step.kind == Step::GROUP) set_error("layers %d..%d: grouped launch failed: %s", step.members.front(), step.members.back(), hipGetErrorString(err));
    else
        set_error("layers %d..%d (%s ...): multi-layer launch failed: %s", step.members.front(), step.members.back(), e->ops[step.lead].name.c_str(),
                  hipGetErrorString(err));
    (void)hipGetLastError();
    return ADAS_ERR_HIP;
}

bool stream_capturing(hipStream_t st) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return false; }
    return cs != hipStreamCaptureStatusNone;
}

}  // namespace

// The schedule's device tables are allocations and copies, so they are never built inside a stream capture: adas_pipeline_* prepares
// before it captures; a forward that finds nothing prepared while capturing runs the plain schedule.
int adas::engine_forward(adas_engine* e, const float* d_in, int batch, hipStream_t st, bool packed_in) {
    if (!e->schedules.count(batch) && !stream_capturing(st)) {
        int rc = engine_prepare(e, batch);
        if (rc != ADAS_OK) return rc;
    }
    Schedule local;
    for (const Step& step : schedule_at(e, batch, &local).steps) {
        int rc = run_step(e, step, d_in, batch, st, packed_in);
        if (rc != ADAS_OK) return rc;
    }
    return ADAS_OK;
}

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
// the multi-layer steps prepared for this batch size (none: nothing prepared, or another mode)
static std::vector<const Step*> ml_steps(const adas_engine* e, int batch) {
    std::vector<const Step*> v;
    auto it = e->schedules.find(batch);
    if (it != e->schedules.end())
        for (auto& st : it->second.steps)
            if (st.kind == Step::ML) v.push_back(&st);
    return v;
}
int adas_engine_ml_info(const adas_engine* e, int batch, int32_t* n_launches, int32_t* n_layers, int32_t* n_items) {
    ADAS_REQUIRE(e && batch > 0, ADAS_ERR_INVALID, "adas_engine_ml_info: bad argument");
    int nl = 0, ni = 0, ns = 0;
    for (const Step* st : ml_steps(e, batch)) { ++ns; nl += (int)st->members.size(); ni += st->ml_items; }
    if (n_launches) *n_launches = ns;
    if (n_layers) *n_layers = nl;
    if (n_items) *n_items = ni;
    return ADAS_OK;
}
int adas_engine_ml_status(const adas_engine* e, int batch, uint32_t* error_word) {
    ADAS_REQUIRE(e && error_word, ADAS_ERR_INVALID, "adas_engine_ml_status: bad argument");
    *error_word = 0;
    for (const Step* st : ml_steps(e, batch)) {
        unsigned w = 0;
        ADAS_REQUIRE(ml_plan_status(st->plan, &w) == 0, ADAS_ERR_HIP, "adas_engine_ml_status: could not read the control block");
        if (w) {
            *error_word = w;
            set_error("multi-layer launch of layers %d..%d: a dependency wait timed out (item %u)", st->members.front(), st->members.back(), w - 1);
            return ADAS_ERR_HIP;
        }
    }
    return ADAS_OK;
}
int adas_engine_ml_counters(const adas_engine* e, int batch, int launch, uint32_t head16[16]) {
    ADAS_REQUIRE(e && head16, ADAS_ERR_INVALID, "adas_engine_ml_counters: bad argument");
    const std::vector<const Step*> steps = ml_steps(e, batch);
    ADAS_REQUIRE(launch >= 0 && launch < (int)steps.size(), ADAS_ERR_INVALID, "adas_engine_ml_counters: no multi-layer launch %d at batch %d", launch, batch);
    unsigned w = 0;
    ADAS_REQUIRE(ml_plan_status(steps[launch]->plan, &w, head16) == 0, ADAS_ERR_HIP, "adas_engine_ml_counters: could not read the control block");
    return ADAS_OK;
}
int adas_engine_launch_count(adas_engine* e, int batch) {
    if (!e || batch <= 0 || batch > e->max_batch) return -1;
    Schedule local;
    return (int)schedule_at(e, batch, &local).steps.size();
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

int adas_debug_h8x3_onepass(const adas_ml_layer_desc* layer, int batch) {
    if (!layer || batch <= 0) return -1;
    ConvArgs a = conv_args_of_desc(*layer, batch, PREC_X3);
    const ConvPlan pl = plan_conv(PREC_X3, a.kh, a.kw, a.stride, a.pad, a.max_n, a.res_mode, a.in, a.out);
    a.kpad = pl.kpad;
    if (wants_x3h8_packing(PREC_X3, pl.kernel, a.kh, a.kw, a.stride, a.pad, a.res_mode, a.in, a.out)) a.wgt_h8x3 = (const void*)(uintptr_t)0x1000;
    return (conv_route(a) == ConvRoute::H8X3 && halo8_x3_onepass(a)) ? 1 : 0;
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
    if (e->mode == adas_engine::ML) {
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
    {
        int rc = engine_prepare(e, batch);
        if (rc != ADAS_OK) return rc;
    }
    const std::vector<Step>& steps = e->schedules.at(batch).steps;
    const size_t n_ev = (steps.size() > 8 ? steps.size() : 8) + 1;   // one ahead of the first step, one behind every step (and 9 for the marker's own cost)
    while (e->events.size() < n_ev) {
        hipEvent_t ev = nullptr;
        ADAS_HIP_TRY(hipEventCreate(&ev));
        e->events.push_back(ev);
    }
    for (int i = 0; i < n; ++i) ms_per_layer[i] = 0.f;
    // an event record is itself a packet on the stream (~5 us between two records with nothing in between): measured here and taken
    // off every step, so that the per-layer sum is the kernels' time, not kernels + markers
    float marker_ms = 0.f;
    {
        const int reps = 8;
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
    // a step's time goes to its lead (the layer adas_engine_layer_kernel labels with the step's kernel); every layer that rides in a
    // launch, or that nothing computes, reads exactly 0
    for (int it = 0; it < iters; ++it) {
        ADAS_HIP_TRY(hipEventRecord(e->events[0], 0));
        for (size_t k = 0; k < steps.size(); ++k) {
            int rc = run_step(e, steps[k], d_input, batch, 0, false);
            if (rc != ADAS_OK) return rc;
            ADAS_HIP_TRY(hipEventRecord(e->events[k + 1], 0));
        }
        ADAS_HIP_TRY(hipStreamSynchronize(0));
        for (size_t k = 0; k < steps.size(); ++k) {
            float ms = 0.f;
            ADAS_HIP_TRY(hipEventElapsedTime(&ms, e->events[k], e->events[k + 1]));
            ms -= marker_ms;
            ms_per_layer[steps[k].lead] += (ms > 0.f ? ms : 0.f) / (float)iters;
        }
    }
    if (num_layers) *num_layers = n;
    return ADAS_OK;
}

int adas_engine_fetch_activation(adas_engine* e, int layer, int batch, float* h_out, int64_t dims[4]) {
    ADAS_REQUIRE(e && layer >= 0 && layer < (int)e->ops.size() && batch > 0 && batch <= e->max_batch, ADAS_ERR_INVALID, "bad layer/batch");
    const FileOp& o = e->ops[layer].f;
    Schedule local;
    const char* why = nullptr;   // why the layer has no activation in memory
    switch (schedule_at(e, batch, &local).role[layer]) {
    case ROLE_IN_DETECT: why = "is fused into the Detect launch and has no materialised activation (ADAS_NO_DETECT_FUSE=1 keeps it)"; break;
    case ROLE_STEM_INPUT:
    case ROLE_STEM_LEAD: why = "is fused into the stem launch and has no materialised activation (ADAS_NO_STEM=1 keeps it)"; break;
    case ROLE_IN_SHORTCUT_USER: why = "is a projection shortcut computed inside the conv that adds it at this batch (ADAS_NO_DS_FUSE=1 keeps it)"; break;
    case ROLE_IN_CONSUMER_LOADS: why = "is folded into its consumer's loads and has no materialised activation (ADAS_NO_UPSAMPLE_FOLD=1 keeps it)"; break;
    case ROLE_C2F_LEAD:   // a fused C2f launch materialises only its cv2 output: cv1 and the Bottleneck's two convs stay in LDS
    case ROLE_C2F_HIDDEN: why = "is computed inside a fused C2f launch: its activation stays in LDS (ADAS_NO_C2F_FUSE=1 keeps it)"; break;
    case ROLE_PAIR_FIRST: why = "is the first conv of a fused 3x3 pair: its activation stays in LDS (ADAS_NO_PAIR_FUSE=1 keeps it)"; break;
    default: break;
    }
    ADAS_REQUIRE(!why, ADAS_ERR_INVALID, "layer %d (%s) %s", layer, e->ops[layer].name.c_str(), why);
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
