// engine_schedule.cpp -- what one forward at a given batch size launches, in which order, and which layers ride in which launch: decided
// once per batch size, in two phases like the loader (engine_load.cpp).
//   plan_schedule     every layer's role, the steps and their members: no HIP call, a pure function of (the load-time plan, batch, the
//                     engine's mode, ADAS_ML_* switches) -- adas_debug_engine_schedule runs it without a device
//   upload_schedule   the device tables of the grouped / multi-layer steps
// engine.cpp's launch loop, the launch count, the labels, the profiler and adas_engine_fetch_activation all read the result.
#include "engine.h"
#include <stdlib.h>
#include <algorithm>
#include <map>
#include <string>
#include <vector>

namespace adas {

// The ConvArgs of op `i` (a plain OP_CONV: not a stem / pair / C2f launch) at this batch, without a folded projection shortcut.
ConvArgs conv_args_of(const adas_engine* e, int i, int batch) {
    const EngOp& op = e->ops[i];
    const FileOp& o = op.f;
    unsigned char* wb = (unsigned char*)e->d_weights;
    ConvArgs a;
    a.in = in_view(e, o);
    a.out = out_view(e, o);
    if (o.res_mode != RES_NONE) a.res = make_view(e, o.res_buf, o.res_coff, o.out_c);
    else { a.res = a.out; a.res.p = nullptr; }
    a.wgt = wb + op.w_off;
    a.bias = (const float*)(wb + op.b_off);
    a.n = batch; a.kh = o.kh; a.kw = o.kw; a.stride = o.stride; a.pad = o.pad; a.act = o.act; a.res_mode = o.res_mode;
    a.k = op.k; a.kpad = op.kpad; a.m = batch * a.out.h * a.out.w; a.max_n = e->max_batch; a.prec = e->prec;
    if (op.has_x3h8) a.wgt_h8x3 = wb + op.x3h8_w_off;
    a.halo_bn = op.halo_bn;
    if (op.up_src >= 0) {
        a.up = in_view(e, e->ops[op.up_src].f);
        a.up_c = (int)e->ops[op.up_src].f.out_c;
    }
    return a;
}

void attach_shortcut(const adas_engine* e, int i, ConvArgs* a) {
    const EngOp& dsop = e->ops[e->ops[i].ds_src];
    unsigned char* wb = (unsigned char*)e->d_weights;
    a->ds_in = in_view(e, dsop.f);
    a->ds_w = wb + dsop.ds_w_off;
    a->ds_bias = (const float*)(wb + dsop.b_off);
}

namespace {

// Does conv `ci` (linked to a projection shortcut) take the shortcut into its own launch at this batch?  Only conv_h8 computes it, so:
// where the conv runs on conv_h8 as it is (asked with its real residual view, the projection's output buffer) and conv_h8 can carry
// this projection.
bool folds_shortcut(const adas_engine* e, int ci, int batch) {
    const EngOp& op = e->ops[ci];
    if (op.ds_src < 0 || op.kernel != CONV_HALO) return false;
    const ConvArgs a = conv_args_of(e, ci, batch);
    return conv_route(a) == ConvRoute::H8 && halo8_ds_applicable(a, in_view(e, e->ops[op.ds_src].f));
}

// Every layer's role before layers share launches: what the load-time plan fused where, and the shortcuts folded at this batch.
std::vector<uint8_t> base_roles(const adas_engine* e, const std::vector<char>& folds) {
    const int n = (int)e->ops.size();
    std::vector<char> in_c2f(n, 0), c2f_tail(n, 0);   // the three convs a fused C2f launch computes besides its cv1; its cv2
    for (auto& q : e->ops)
        for (int k = 0; k < 3 && q.c2f[0] >= 0; ++k) { in_c2f[q.c2f[k]] = 1; c2f_tail[q.c2f[k]] = k == 2; }
    std::vector<uint8_t> role(n);
    for (int i = 0; i < n; ++i) {
        const EngOp& op = e->ops[i];
        const FileOp& o = op.f;
        const bool conv = o.type == OP_CONV;
        role[i] = conv && op.ds_user >= 0 && folds[op.ds_user]                                ? ROLE_IN_SHORTCUT_USER
                  : op.skip && o.type == OP_UPSAMPLE2                                         ? ROLE_IN_CONSUMER_LOADS
                  : op.skip && o.type == OP_MAXPOOL && (o.kh == 5 || o.kh == 9 || o.kh == 13) ? ROLE_IN_POOL3
                  : conv && op.c2f[0] >= 0                                                    ? ROLE_C2F_LEAD
                  : op.skip && conv && in_c2f[i]                                              ? (c2f_tail[i] ? ROLE_C2F_TAIL : ROLE_C2F_HIDDEN)
                  : op.skip && op.kernel == CONV_PAIR                                         ? ROLE_IN_PAIR
                  : conv && op.pair_b >= 0                                                    ? ROLE_PAIR_FIRST
                  : op.skip && conv && o.kh == 1 && (op.kernel == CONV_PW || op.kernel == CONV_DET5) ? ROLE_IN_DETECT
                  : op.skip                                                                   ? (o.type == OP_INPUT ? ROLE_STEM_INPUT : ROLE_STEM_TAIL)
                  : conv && op.kernel == CONV_STEM && (op.fuse_pool >= 0 || op.fuse_conv2 >= 0) ? ROLE_STEM_LEAD
                                                                                              : ROLE_OWN;
    }
    return role;
}

// Layer `i` on its own kernel, and what the load-time plan (or, for a shortcut, this batch) put into its launch.
Step op_step(const adas_engine* e, int i, bool folds) {
    const EngOp& op = e->ops[i];
    Step st;
    st.lead = i;
    st.folds_shortcut = folds;
    st.members.push_back(i);
    auto rides = [&](int j) { if (j >= 0) st.members.push_back(j); };
    if (op.f.type == OP_CONV && op.kernel == CONV_STEM) {
        if (e->ops[0].skip) rides(0);
        rides(op.fuse_pool); rides(op.fuse_conv2);
    }
    if (folds) rides(op.ds_src);
    for (int j : op.pool3) rides(j);
    rides(op.pair_b);
    for (int j : op.c2f) rides(j);
    for (int j : op.det_src) rides(j);
    return st;
}

// Is op `i` a conv that launches on its own at this batch, untouched by any fusion and clear of aliased buffers -- what both kinds of
// shared launch start from?  Then *a are its arguments.
bool shareable_conv(const adas_engine* e, const std::vector<uint8_t>& role, const std::vector<char>& folds, int i, int batch, ConvArgs* a) {
    const EngOp& op = e->ops[i];
    const FileOp& o = op.f;
    if (role[i] != ROLE_OWN || o.type != OP_CONV || (op.kernel != CONV_HALO && op.kernel != CONV_PW)) return false;
    if (folds[i]) return false;   // carries its projection: conv_halo8 only
    auto aliased = [&](int b) { return b >= 0 && b < (int)e->buf_aliased.size() && e->buf_aliased[b]; };
    if (aliased(o.in_buf[0]) || aliased(o.out_buf) || (o.res_mode != RES_NONE && aliased(o.res_buf))) return false;
    if (op.up_src >= 0 && aliased(e->ops[op.up_src].f.in_buf[0])) return false;
    *a = conv_args_of(e, i, batch);
    return true;
}

int env_int(const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
}

// Maximal runs of consecutive candidates, at most ML_MAX_LAYERS long: layers that launch nothing are transparent, any other layer ends
// the run.  emit(ops, layers) gets every run of at least min_layers.
template <class Cand, class Emit>
void scan_runs(const std::vector<uint8_t>& role, int min_layers, Cand cand, Emit emit) {
    const int n = (int)role.size();
    int i = 0;
    while (i < n) {
        std::vector<ConvArgs> layers;
        std::vector<int> ops;
        int j = i, last = i;
        for (; j < n; ++j) {
            if (!role_launches(role[j])) continue;
            ConvArgs a;
            if ((int)layers.size() >= ML_MAX_LAYERS || !cand(j, &a)) break;
            layers.push_back(a); ops.push_back(j);
            last = j;
        }
        if ((int)layers.size() >= min_layers) emit(ops, layers);
        i = (layers.empty() ? j : last) + 1;
    }
}

void index_steps(Schedule* s) {
    std::fill(s->step_of.begin(), s->step_of.end(), -1);
    for (size_t k = 0; k < s->steps.size(); ++k)
        for (int m : s->steps[k].members) s->step_of[m] = (int)k;
}

void release_tables(Step* st) {
    ml_group_destroy(st->group);
    ml_plan_destroy(st->plan);
    st->group = nullptr; st->plan = nullptr;
}

// The steps of run `run` give way to one OP step per layer, in layer order (its tables could not be allocated).
void unshare_run(Schedule* s, int run) {
    std::vector<Step> out;
    std::vector<int> layers;
    size_t at = 0;
    for (auto& st : s->steps) {
        if (st.run != run) { out.push_back(st); continue; }
        if (layers.empty()) at = out.size();
        release_tables(&st);
        layers.insert(layers.end(), st.members.begin(), st.members.end());
    }
    std::sort(layers.begin(), layers.end());
    for (size_t k = 0; k < layers.size(); ++k) {
        Step st;
        st.lead = layers[k];
        st.members.push_back(layers[k]);
        out.insert(out.begin() + at + k, st);
        s->role[layers[k]] = ROLE_OWN;
    }
    s->steps.swap(out);
    index_steps(s);
}

}  // namespace

Schedule plan_schedule(const adas_engine* e, int batch, bool fused_launches) {
    const int n = (int)e->ops.size();
    std::vector<char> folds(n, 0);
    for (int i = 0; i < n; ++i) folds[i] = folds_shortcut(e, i, batch);
    Schedule s;
    s.role = base_roles(e, folds);
    s.step_of.assign(n, -1);
    struct Run { int last; std::vector<Step> steps; };
    std::map<int, Run> runs;   // by first layer
    int n_runs = 0;
    if (fused_launches && e->mode == adas_engine::GROUPED) {
        // 3x3 convs that launch on conv_halo at this batch, level by level: the independent layers of a level share a launch
        auto cand = [&](int i, ConvArgs* a) {
            return shareable_conv(e, s.role, folds, i, batch, a) && e->ops[i].kernel == CONV_HALO && e->ops[i].up_src < 0 && group_layer_supported(*a, CONV_HALO);
        };
        scan_runs(s.role, 2, cand, [&](const std::vector<int>& ops, const std::vector<ConvArgs>& layers) {
            const std::vector<int> level = ml_levels(layers);
            const int nlev = 1 + *std::max_element(level.begin(), level.end());
            Run run{ops.back(), {}};
            bool any_group = false;
            for (int lv = 0; lv < nlev; ++lv) {
                std::vector<int> at;
                for (size_t k = 0; k < ops.size(); ++k)
                    if (level[k] == lv) at.push_back(ops[k]);
                for (size_t c0 = 0; c0 < at.size(); c0 += ML_GROUP_MAX) {   // at most ML_GROUP_MAX layers per launch
                    const size_t c1 = std::min(c0 + ML_GROUP_MAX, at.size());
                    Step st = op_step(e, at[c0], false);
                    if (c1 - c0 >= 2) {
                        st.kind = Step::GROUP;
                        st.members.assign(at.begin() + c0, at.begin() + c1);
                        any_group = true;
                    }
                    st.run = n_runs;
                    run.steps.push_back(st);
                }
            }
            if (!any_group) return;   // a chain: every layer its own launch, in layer order
            ++n_runs;
            runs[ops.front()] = run;
        });
    } else if (fused_launches && e->mode == adas_engine::ML) {
        // convs with a tile body in the multi-layer kernel (conv_ml.hip); experiments: ADAS_ML_ONLY=halo | pw keeps the other kind of
        // layer out, ADAS_ML_MAX_LAYER_ITEMS layers with more items, ADAS_ML_MIN_LAYERS shorter runs
        const char* only = getenv("ADAS_ML_ONLY");
        const int max_items = env_int("ADAS_ML_MAX_LAYER_ITEMS", 0);
        auto cand = [&](int i, ConvArgs* a) {
            const int kernel = e->ops[i].kernel;
            if (only && ((only[0] == 'h' && kernel != CONV_HALO) || (only[0] == 'p' && kernel != CONV_PW))) return false;
            if (!shareable_conv(e, s.role, folds, i, batch, a) || !ml_layer_supported(*a, kernel)) return false;
            return max_items <= 0 || (long)((a->m + 255) / 256) * ((a->out.c + 63) / 64) <= max_items;
        };
        scan_runs(s.role, std::max(1, env_int("ADAS_ML_MIN_LAYERS", 2)), cand, [&](const std::vector<int>& ops, const std::vector<ConvArgs>& layers) {
            std::vector<int> kernels;
            for (int m : ops) kernels.push_back(e->ops[m].kernel);
            std::string why;
            MlPlanInfo info;
            MlPlan* pl = ml_plan_create(layers, kernels, e->prec, &why, &info, true);
            if (!pl) return;          // (too many producers for one item ...): the layers keep their own launches
            ml_plan_destroy(pl);
            Step st;
            st.kind = Step::ML;
            st.lead = ops.front();
            st.members = ops;
            st.run = n_runs++;
            st.ml_items = info.n_items;
            runs[ops.front()] = Run{ops.back(), {st}};
        });
    }
    for (int i = 0; i < n; ++i) {
        auto it = runs.find(i);
        if (it != runs.end()) {
            s.steps.insert(s.steps.end(), it->second.steps.begin(), it->second.steps.end());
            i = it->second.last;
        } else if (role_launches(s.role[i])) {
            s.steps.push_back(op_step(e, i, folds[i]));
        }
    }
    for (auto& st : s.steps)
        for (int m : st.members)
            if (st.kind != Step::OP) s.role[m] = st.kind == Step::GROUP ? (m == st.lead ? ROLE_GROUP_LEAD : ROLE_GROUP_MEMBER) : (m == st.lead ? ROLE_ML_LEAD : ROLE_ML_MEMBER);
    index_steps(&s);
    return s;
}

namespace {
// The allocations and copies of upload_schedule must not land in -- or invalidate -- a stream capture the calling thread has open on
// ANOTHER stream (engine_forward only knows its own): they run with the thread's capture mode relaxed, restored on every exit.
struct RelaxedCaptureMode {
    hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
    bool ok;
    RelaxedCaptureMode() { ok = hipThreadExchangeStreamCaptureMode(&mode) == hipSuccess; if (!ok) (void)hipGetLastError(); }
    ~RelaxedCaptureMode() { if (ok && hipThreadExchangeStreamCaptureMode(&mode) != hipSuccess) (void)hipGetLastError(); }
};
}  // namespace

void upload_schedule(const adas_engine* e, int batch, Schedule* s) {
    RelaxedCaptureMode relaxed;
    for (size_t k = 0; k < s->steps.size(); ++k) {
        Step& st = s->steps[k];
        if (st.kind == Step::OP || st.group || st.plan) continue;
        std::vector<ConvArgs> layers;
        std::vector<int> kernels;
        for (int m : st.members) { layers.push_back(conv_args_of(e, m, batch)); kernels.push_back(e->ops[m].kernel); }
        std::string why;
        if (st.kind == Step::GROUP) st.group = ml_group_create(layers, e->prec, &why);
        else st.plan = ml_plan_create(layers, kernels, e->prec, &why);
        if (st.group || st.plan) continue;
        unshare_run(s, st.run);   // the device allocation failed: the whole run on per-layer launches
        k = (size_t)-1;           // (the steps moved: from the start again, past what is uploaded)
    }
}

void free_schedule(Schedule* s) {
    for (auto& st : s->steps) release_tables(&st);
}

// Tables are kept for the life of the engine (a captured hipGraph may reference them): at most this many distinct batch sizes get
// them, later ones run one launch per layer.
constexpr size_t kMaxPreparedBatches = 16;

int engine_prepare(adas_engine* e, int batch) {
    if (e->schedules.count(batch)) return ADAS_OK;
    const bool fused = e->mode != adas_engine::PLAIN && e->schedules.size() < kMaxPreparedBatches;
    Schedule s = plan_schedule(e, batch, fused);
    if (fused) upload_schedule(e, batch, &s);
    e->schedules.emplace(batch, std::move(s));
    return ADAS_OK;
}

const Schedule& schedule_at(const adas_engine* e, int batch, Schedule* local) {
    auto it = e->schedules.find(batch);
    if (it != e->schedules.end()) return it->second;
    *local = plan_schedule(e, batch, false);
    return *local;
}

void layer_label(const adas_engine* e, const Schedule& s, int layer, int batch, char* name, int cap) {
    const EngOp& op = e->ops[layer];
    const FileOp& o = op.f;
    static const char* kOther[] = {"input_nchw_kernel", "", "maxpool_kernel", "upsample2_kernel", "detect_v8_kernel", "detect_v5_kernel",
                                   "layernorm_kernel", "dwconv_kernel", "attention_kernel", "avgpool_kernel", "depth2space_kernel", "detect_v6_kernel",
                                   "se_gate_kernel", "scale_kernel", "wsum_kernel", "shuffle_kernel"};
    const Step* st = s.step_of[layer] >= 0 ? &s.steps[s.step_of[layer]] : nullptr;
    switch (s.role[layer]) {
    case ROLE_GROUP_LEAD: snprintf(name, cap, "conv_halo_group_kernel[%d layers]", (int)st->members.size()); return;
    case ROLE_GROUP_MEMBER: snprintf(name, cap, "(in the grouped launch)"); return;
    case ROLE_ML_LEAD: snprintf(name, cap, "conv_ml_kernel[%d layers]", (int)st->members.size()); return;
    case ROLE_ML_MEMBER: snprintf(name, cap, "(in the multi-layer launch)"); return;
    case ROLE_IN_SHORTCUT_USER: snprintf(name, cap, "(fused into the conv it is the shortcut of)"); return;
    case ROLE_IN_CONSUMER_LOADS: snprintf(name, cap, "(folded into the consumer's loads)"); return;
    case ROLE_IN_POOL3: snprintf(name, cap, "(fused into the SPPF pool launch)"); return;
    case ROLE_C2F_HIDDEN:
    case ROLE_C2F_TAIL: snprintf(name, cap, "(fused into the C2f launch)"); return;
    case ROLE_IN_PAIR: snprintf(name, cap, "(fused into the pair launch)"); return;
    case ROLE_IN_DETECT: snprintf(name, cap, "(fused into the Detect launch)"); return;
    case ROLE_STEM_INPUT:
    case ROLE_STEM_TAIL: snprintf(name, cap, "(fused into the stem launch)"); return;
    case ROLE_C2F_LEAD: snprintf(name, cap, e->prec == PREC_X3 ? "conv_c2f16_x3_kernel" : "conv_c2f16_kernel"); return;
    case ROLE_PAIR_FIRST: snprintf(name, cap, "conv_pair_kernel<%d>", (int)o.out_c); return;
    default: break;   // ROLE_OWN, ROLE_STEM_LEAD: the kernel of the layer's own type
    }
    if (o.type == OP_MAXPOOL && op.pool3[0] >= 0) {
        snprintf(name, cap, "sppf_pool3_kernel");
    } else if (o.type == OP_CONV && op.kernel == CONV_STEM && op.fuse_conv2 >= 0) {
        snprintf(name, cap, e->prec == PREC_X3 ? "conv_stem2_x3_kernel<%d>+conv3x3s2" : "conv_stem_kernel<%d,1,SILU>+conv3x3s2", (int)o.kh);
    } else if (o.type == OP_CONV) {
        ConvArgs a = conv_args_of(e, layer, batch);
        if (st->folds_shortcut) attach_shortcut(e, layer, &a);
        snprintf(name, cap, "%s%s%s", conv_kernel_name(a, op.kernel == CONV_STEM), op.fuse_pool >= 0 ? "+pool" : "", st->folds_shortcut ? "+shortcut" : "");
    } else if (o.type == OP_DETECT_V8 && op.det_src[0] >= 0) {
        snprintf(name, cap, e->prec == PREC_X3 ? "detect_v8_fused_x3_kernel" : "detect_v8_fused_kernel");
    } else if (o.type == OP_DETECT_V5 && op.det_src[0] >= 0) {
        snprintf(name, cap, "detect_v5_fused_kernel");
    } else if (o.type == OP_DETECT_V6 && o.params[5] != 0.0f) {
        snprintf(name, cap, "detect_v6_dfl_kernel");
    } else {
        snprintf(name, cap, "%s", o.type < 16 ? kOther[o.type] : "?");
    }
}

int write_schedule_rows(const adas_engine* e, const Schedule& s, int batch, int32_t* step_of, int32_t* role, char* labels, int cap, int32_t* n_ops,
                        int32_t* n_steps) {
    const int n = (int)e->ops.size();
    if (n_ops) *n_ops = n;
    if (n_steps) *n_steps = (int32_t)s.steps.size();
    if (!step_of && !role && !labels) return ADAS_OK;
    ADAS_REQUIRE(cap >= n, ADAS_ERR_CAPACITY, "engine schedule: %d layers, room for %d", n, cap);
    for (int i = 0; i < n; ++i) {
        if (step_of) step_of[i] = s.step_of[i];
        if (role) role[i] = s.role[i];
        if (labels) layer_label(e, s, i, batch, labels + (size_t)i * ADAS_LABEL_CAP, ADAS_LABEL_CAP);
    }
    return ADAS_OK;
}

}  // namespace adas

extern "C" int adas_engine_schedule(const adas_engine* e, int batch, int32_t* step_of, int32_t* role, int cap, int32_t* n_ops, int32_t* n_steps) {
    ADAS_REQUIRE(e && batch > 0 && batch <= e->max_batch, ADAS_ERR_INVALID, "adas_engine_schedule: bad argument (batch %d, max %d)", batch, e ? e->max_batch : 0);
    adas::Schedule local;
    return adas::write_schedule_rows(e, adas::schedule_at(e, batch, &local), batch, step_of, role, nullptr, cap, n_ops, n_steps);
}
