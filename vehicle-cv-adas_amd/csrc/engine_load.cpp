// engine_load.cpp -- adas_engine_create: loads an ADASHIP1 model container in four phases.
//   read_container       header, magic, the buffer / operator / output tables
//   validate_container   every refusal of a container, before a byte of device memory is asked for
//   plan_engine          the fusion passes and the weight arena's layout: no HIP call, a pure function of (tables, precision, max_batch,
//                        ADAS_NO_* switches) -- adas_debug_engine_plan runs the first three phases without a device
//   allocate_and_upload  activation buffers, the weight arena, weights packed on the device, the launch schedule of max_batch
// Memory plan: every graph buffer gets its own HBM allocation sized for max_batch frames (the nets are tiny against 288 GB); weights are
// packed once on the device into the compute type with K padded to 32 and Cout to 128 so the conv kernel needs no bounds checks on the
// weight side.
#include "engine.h"
#include <errno.h>
#include <string.h>
#include <memory>
#include <string>
#include <vector>

using namespace adas;

namespace {

// A container's bytes: the model file (closed when the object goes), or the tables in memory.
struct Source {
    FILE* f = nullptr;
    const unsigned char* mem = nullptr;
    size_t size = 0, pos = 0;
    Source() = default;
    Source(const void* p, size_t bytes) : mem((const unsigned char*)p), size(bytes) {}
    Source(const Source&) = delete;
    ~Source() { if (f) fclose(f); }
    bool open(const char* path) {
        f = fopen(path, "rb");
        if (!f) return false;
        if (fseek(f, 0, SEEK_END) == 0) size = (size_t)ftell(f);
        rewind(f);
        return true;
    }
    bool read(void* dst, size_t bytes) {
        if (bytes > size - pos) return false;
        if (f) {
            if (fread(dst, 1, bytes, f) != bytes) return false;
        } else if (bytes) {
            memcpy(dst, mem + pos, bytes);
        }
        pos += bytes;
        return true;
    }
    bool read_at(uint64_t off, void* dst, size_t bytes) {
        if (off > size || (f && fseek(f, (long)off, SEEK_SET) != 0)) return false;
        pos = (size_t)off;
        return read(dst, bytes);
    }
};

struct EngineFree { void operator()(adas_engine* e) const { free_engine(e); } };
using EnginePtr = std::unique_ptr<adas_engine, EngineFree>;   // the engine under construction: freed unless it is released to the caller

std::string fixed_name(const char* s, size_t cap) { return std::string(s, strnlen(s, cap)); }

// ---- phase 1: header, magic, tables.  `on_device`: the engine will run, so a device must be visible (asked after the magic check)
int read_container(Source& src, const char* label, bool on_device, int precision, int max_batch, EnginePtr& e) {
    FileHeader hd;
    ADAS_REQUIRE(src.read(&hd, sizeof(hd)) && memcmp(hd.magic, "ADASHIP1", 8) == 0 && hd.version == 1, ADAS_ERR_FORMAT,
                 "[%s] is not an ADASHIP1 model container (convert an ONNX export with vehicle-cv-adas_amd/onnx_import.py or "
                 "build one with models.py; TensorRT plans cannot be imported)", label);
    ADAS_REQUIRE(!on_device || adas_device_count() > 0, ADAS_ERR_NO_DEVICE, "no HIP device visible; this library has no CPU fallback");
    e.reset(new adas_engine());
    e->prec = precision;
    e->max_batch = max_batch;
    // multi-layer launches are opt-in (ADAS_ML=1): measured slower than the per-layer launches at 64 frames (profiles/r05/ml_*.txt)
    e->mode = !prec_is16(precision) ? adas_engine::PLAIN : env_on("ADAS_ML") ? adas_engine::ML : env_on("ADAS_NO_GROUP") ? adas_engine::PLAIN : adas_engine::GROUPED;
    e->hdr = hd;
    e->name = fixed_name(hd.name, sizeof(hd.name));
    const uint64_t table_bytes = (uint64_t)hd.n_bufs * sizeof(FileBuf) + (uint64_t)hd.n_ops * sizeof(FileOp) + (uint64_t)hd.n_outputs * sizeof(FileOut);
    std::vector<FileBuf> fb;
    std::vector<FileOp> fo;
    std::vector<FileOut> fout;
    bool ok = table_bytes <= src.size - src.pos;   // (before the tables are sized by what a damaged header claims)
    if (ok) {
        fb.resize(hd.n_bufs); fo.resize(hd.n_ops); fout.resize(hd.n_outputs);
        ok = src.read(fb.data(), fb.size() * sizeof(FileBuf)) && src.read(fo.data(), fo.size() * sizeof(FileOp)) && src.read(fout.data(), fout.size() * sizeof(FileOut));
    }
    ADAS_REQUIRE(ok, ADAS_ERR_FORMAT, "[%s]: truncated model container", label);
    for (auto& b : fb) {
        EngBuf eb;
        eb.h = b.h; eb.w = b.w; eb.c = b.c; eb.f32 = (b.flags & 1) != 0; eb.d = nullptr;
        eb.alias_of = (b.flags & 2) ? (int)(b.flags >> 8) : -1;
        e->bufs.push_back(eb);
    }
    for (auto& o : fo) {
        EngOp op;
        op.f = o;
        op.name = fixed_name(o.name, sizeof(o.name));
        e->ops.push_back(op);
    }
    for (auto& o : fout) {
        EngOut eo;
        eo.buf = o.buf; eo.offset = o.offset; eo.ndim = o.ndim;
        for (int i = 0; i < 4; ++i) eo.dims[i] = o.dims[i];
        eo.elems = 1;
        for (int i = 1; i < (int)o.ndim && i < 4; ++i) eo.elems *= o.dims[i];
        eo.name = fixed_name(o.name, sizeof(o.name));
        e->outs.push_back(eo);
    }
    return ADAS_OK;
}

// The operators without a generic fallback must be shapes their kernel takes (a damaged or foreign container fails here, not at launch).
bool op_shape_ok(const adas_engine* e, const FileOp& o) {
    const TView out = out_view(e, o);
    switch (o.type) {
    case OP_DWCONV:
        return o.n_in == 1 && o.kh == o.kw && dwconv_supported((int)o.kh, (int)o.stride, (int)o.pad, (int)o.res_mode, in_view(e, o), out) &&
               o.w_elems == (uint64_t)o.kh * o.kw * o.out_c && o.b_elems == (uint64_t)o.out_c;
    case OP_ATTENTION: return o.n_in == 1 && attention_supported((int)o.params[0], (int)o.params[1], (int)o.params[2], in_view(e, o), out);
    case OP_DEPTH2SPACE: return o.n_in == 1 && depth2space_supported(in_view(e, o), out);
    case OP_DETECT_V6: return o.n_in == 6;
    case OP_SE_GATE: return o.n_in == 1 && se_gate_supported(in_view(e, o), out, (int)o.params[0], o.w_elems, o.b_elems);
    case OP_SCALE: return o.n_in == 2 && scale_supported(in_view(e, o, 0), in_view(e, o, 1), out);
    case OP_SHUFFLE: return o.n_in == 1 && shuffle_supported(in_view(e, o), out, (int)o.params[0]);
    case OP_WSUM: {
        TView ins[3];
        for (uint32_t k = 0; k < o.n_in && k < 3; ++k) ins[k] = in_view(e, o, k);
        return o.n_in <= 3 && wsum_supported((int)o.n_in, ins, out) && o.act <= ACT_RELU6;
    }
    default: return true;
    }
}

const char* op_shape_name(uint32_t type) {
    return type == OP_DWCONV ? "depth-wise convolution" : type == OP_ATTENTION ? "attention" : type == OP_DEPTH2SPACE ? "depth-to-space"
           : type == OP_SE_GATE ? "squeeze-and-excitation" : type == OP_SCALE ? "channel scale" : type == OP_WSUM ? "weighted sum"
           : type == OP_SHUFFLE ? "channel shuffle" : "Detect";
}

// ---- phase 2: every refusal that needs no plan ("a Linear layer cannot carry a residual" needs plan_conv: layout_arena, still before
// the first allocation)
int validate_container(adas_engine* e, const char* label) {
    {   // every buffer index an op or output names must exist (a damaged container must not index past e->bufs)
        auto bad = [&](int64_t b) { return b < 0 || b >= (int64_t)e->bufs.size(); };
        const char* what = nullptr;
        for (auto& op : e->ops) {
            const FileOp& o = op.f;
            if (o.n_in > 8) { what = "more than 8 inputs"; break; }
            for (uint32_t k = 0; k < o.n_in; ++k)
                if (bad(o.in_buf[k])) what = "input buffer";
            if (bad(o.out_buf)) what = "output buffer";
            if (o.res_mode != RES_NONE && bad(o.res_buf)) what = "residual buffer";
            if (what) break;
        }
        for (auto& q : e->outs)
            if (bad(q.buf)) what = "graph output buffer";
        ADAS_REQUIRE(!what, ADAS_ERR_FORMAT, "[%s]: %s index out of range (container has %u buffers)", label, what, e->hdr.n_bufs);
    }
    e->buf_aliased.assign(e->bufs.size(), 0);
    for (size_t bi = 0; bi < e->bufs.size(); ++bi) {  // an alias re-declares the shape of an EARLIER buffer's memory (torch .view)
        const EngBuf& b = e->bufs[bi];
        if (b.alias_of < 0) continue;
        const bool ok = b.alias_of < (int)bi && e->bufs[b.alias_of].alias_of < 0 &&
                        (size_t)b.h * b.w * b.c == (size_t)e->bufs[b.alias_of].h * e->bufs[b.alias_of].w * e->bufs[b.alias_of].c &&
                        b.f32 == e->bufs[b.alias_of].f32;
        ADAS_REQUIRE(ok, ADAS_ERR_FORMAT, "[%s]: buffer %zu is not a valid alias", label, bi);
        e->buf_aliased[bi] = e->buf_aliased[b.alias_of] = 1;
    }
    if (e->prec == PREC_X3)   // the G8 layout groups 8 channels: every 16-bit tensor of the graph must be a whole number of groups
        for (size_t bi = 0; bi < e->bufs.size(); ++bi)
            ADAS_REQUIRE(e->bufs[bi].f32 || !(e->bufs[bi].c & 7), ADAS_ERR_FORMAT,
                         "[%s]: buffer %zu has %d channels: the split precision (fp16x3) needs multiples of 8", label, bi, e->bufs[bi].c);
    Placeholders ids(e);
    for (auto& op : e->ops) {
        const FileOp& o = op.f;
        if (o.type == OP_DETECT_V6 && o.n_in == 6) {   // params[5] = reg_max: 0 = 4 distances (containers before DFL carry 0), 16 = DFL bins
            const float rm = o.params[5];
            ADAS_REQUIRE(rm == 0.0f || rm == 16.0f, ADAS_ERR_FORMAT,
                         "[%s]: layer %s: YOLOv6 Detect: reg_max %g is not supported (0: 4 distance channels; 16: 4 x 17 DFL bins)", label, op.name.c_str(), (double)rm);
            for (int l = 0; l < 3; ++l)
                ADAS_REQUIRE(o.in_c[2 * l] == 4 * ((int)rm + 1), ADAS_ERR_FORMAT,
                             "[%s]: layer %s: YOLOv6 Detect: level %d regression input has %d channels, reg_max %d needs 4 x (reg_max + 1) = %d", label,
                             op.name.c_str(), l, o.in_c[2 * l], (int)rm, 4 * ((int)rm + 1));
        }
        // hard-swish / hard-sigmoid: element-wise layers only (kernels.h)
        ADAS_REQUIRE(!((o.type == OP_CONV || o.type == OP_DWCONV) && o.act > ACT_LEAKY), ADAS_ERR_FORMAT,
                     "[%s]: layer %s: activation %u is not a convolution epilogue (lower it as a one-input weighted-sum layer)", label, op.name.c_str(), o.act);
        ADAS_REQUIRE(op_shape_ok(e, o), ADAS_ERR_FORMAT, "[%s]: layer %s: unsupported %s shape", label, op.name.c_str(), op_shape_name(o.type));
    }
    for (auto& o : e->outs) ADAS_REQUIRE(e->bufs[o.buf].f32, ADAS_ERR_FORMAT, "[%s]: output %s is not an fp32 buffer", label, o.name.c_str());
    return ADAS_OK;
}

// ---- who uses a tensor: the one statement of the questions the fusion passes ask of the operator and output tables.  The passes count
// readers by buffer index; a buffer that is re-viewed through an alias (Graph.alias: the same bytes under another shape) has readers those
// counts would miss, so every pass keeps aliased() buffers out.
struct Uses {
    const adas_engine* e;
    struct Readers { int count = 0, last = -1; };
    const FileOp& op(int i) const { return e->ops[i].f; }
    int n_ops() const { return (int)e->ops.size(); }
    // does q read buffer `buf` as an input or as its residual -- c < 0: any part of it; else: channels [coff, coff + c) of it
    static bool reads(const FileOp& q, int buf, int coff = 0, int c = -1) {
        auto hit = [&](int b, int o, int n) { return b == buf && (c < 0 || (o < coff + c && o + n > coff)); };
        bool r = q.res_mode != RES_NONE && hit(q.res_buf, q.res_coff, q.out_c);
        for (uint32_t t = 0; t < q.n_in; ++t) r = r || hit(q.in_buf[t], q.in_coff[t], q.in_c[t]);
        return r;
    }
    Readers readers(int buf, int except = -1, int coff = 0, int c = -1) const {   // how many ops (other than `except`) read it, and the last of them
        Readers r;
        for (int j = 0; j < n_ops(); ++j)
            if (j != except && reads(op(j), buf, coff, c)) { ++r.count; r.last = j; }
        return r;
    }
    bool is_output(int buf) const {
        for (auto& q : e->outs)
            if ((int)q.buf == buf) return true;
        return false;
    }
    bool aliased(int buf) const { return buf >= 0 && buf < (int)e->buf_aliased.size() && e->buf_aliased[buf]; }
    int producer(int buf, int coff, int c, int before) const {   // the last conv ahead of op `before` that writes exactly this view, or -1
        for (int j = before - 1; j >= 0; --j)
            if (op(j).type == OP_CONV && op(j).out_buf == buf && op(j).out_coff == coff && op(j).out_c == c) return j;
        return -1;
    }
    bool written_between(int buf, int i, int j) const {   // by an op strictly between ops i and j
        for (int k = i + 1; k < j; ++k)
            if (op(k).out_buf == buf) return true;
        return false;
    }
};

bool feeds(const FileOp& a, const FileOp& b) { return b.in_buf[0] == a.out_buf && b.in_coff[0] == a.out_coff && b.in_c[0] == a.out_c; }

// ---- pass 1, first-layer fusion (conv_stem.hip, conv_stem_x3.hip): input conversion + stride-2 conv in one launch, and with them the
// ResNet stem's max-pool or the YOLO stems' 3x3 s2 conv on the stem's 16 channels, when nothing else reads the stem's output
void fuse_stem(adas_engine* e, const Uses& u) {
    if (env_on("ADAS_NO_STEM") || e->ops.size() < 2) return;
    const FileOp &in = e->ops[0].f, &c1 = e->ops[1].f;
    if (in.type != OP_INPUT || c1.type != OP_CONV || c1.in_buf[0] != in.out_buf || u.aliased(in.out_buf) || u.aliased(c1.out_buf)) return;
    // the facts both precisions' stems ask for
    const bool only = u.readers(in.out_buf).last < 2;                    // the conv is the input's only reader
    const FileOp* q2 = e->ops.size() >= 3 ? &e->ops[2].f : nullptr;     // the op that may join the launch
    const bool sole = q2 && feeds(c1, *q2) && !u.is_output(c1.out_buf) && u.readers(c1.out_buf).last < 3;   // ... the conv output's only reader
    const bool pool_cand = sole && q2->type == OP_MAXPOOL && q2->kh == 3 && q2->stride == 2 && q2->pad == 1;
    const bool conv_cand = sole && q2->type == OP_CONV;
    const TView cv = out_view(e, c1);
    const int prec = e->prec, in_c = (int)e->hdr.in_c;
    bool pool = pool_cand, conv2 = false;
    if (prec == PREC_X3) {   // conv_stem_x3.hip
        if (!only || !stem_x3_applicable(in_c, c1.kh, c1.kw, c1.stride, c1.pad, c1.act, c1.res_mode, cv)) return;
        pool = pool && !u.aliased(q2->out_buf) && !env_on("ADAS_NO_STEM_POOL_X3") &&
               stem_pool_x3_applicable(in_c, c1.kh, c1.kw, c1.stride, c1.pad, c1.act, c1.res_mode, cv, out_view(e, *q2));
        conv2 = !pool && conv_cand && q2->n_in == 1 && !u.aliased(q2->out_buf) &&
                stem2_x3_applicable(in_c, c1.kh, c1.pad, c1.act, cv, q2->kh, q2->kw, q2->stride, q2->pad, q2->act, q2->res_mode, out_view(e, *q2));
    } else {                 // conv_stem.hip: the stem with the pool is a launch of its own kind, asked for first
        const TView pv = pool ? out_view(e, *q2) : cv;
        pool = pool && stem_applicable(prec, in_c, c1.kh, c1.kw, c1.stride, c1.pad, c1.act, c1.res_mode, cv, true, pv);
        if (!only || !stem_applicable(prec, in_c, c1.kh, c1.kw, c1.stride, c1.pad, c1.act, c1.res_mode, cv, pool, pool ? pv : cv)) return;
        conv2 = !pool && !env_on("ADAS_NO_STEM2") && conv_cand &&
                stem2_applicable(prec, c1.kh, c1.pad, c1.act, cv, q2->kh, q2->kw, q2->stride, q2->pad, q2->act, q2->res_mode, out_view(e, *q2));
    }
    e->ops[0].skip = true;
    e->ops[1].kernel = CONV_STEM;
    if (pool) e->ops[1].fuse_pool = 2;
    if (conv2) {
        e->ops[1].fuse_conv2 = 2;
        e->ops[2].kernel = CONV_STEM2;
    }
    if (pool || conv2) e->ops[2].skip = true;
}

// ---- pass 2, projection shortcut folded into the conv that adds it (ResNet layerN.0: conv2 + downsample).  Only the link is made here:
// whether a launch takes it is decided per batch, because the kernel that can (conv_halo8.hip) is chosen by batch (engine_schedule.cpp folds_shortcut)
void link_shortcuts(adas_engine* e, const Uses& u) {
    for (int ci = 0; ci < u.n_ops() && prec_is16(e->prec); ++ci) {
        const FileOp& c = u.op(ci);
        if (c.type != OP_CONV || c.kh != 3 || c.kw != 3 || c.stride != 1 || c.pad != 1 || c.res_mode != RES_BEFORE_ACT) continue;
        const int di = u.producer(c.res_buf, c.res_coff, c.out_c, ci);
        if (di < 0) continue;
        const FileOp& d = u.op(di);
        if (d.kh != 1 || d.kw != 1 || d.stride != 2 || d.pad != 0 || d.act != ACT_NONE || d.res_mode != RES_NONE || d.n_in != 1 || (d.in_c[0] & 31) ||
            (d.out_c & 63) || e->ops[di].skip)
            continue;
        // the conv is the projection's one reader, and x is not rewritten between the two
        if (u.readers(d.out_buf).count != 1 || u.is_output(d.out_buf) || u.written_between(d.in_buf[0], di, ci) || u.aliased(d.out_buf)) continue;
        e->ops[ci].ds_src = di;
        e->ops[di].ds_user = ci;
    }
}

// ---- pass 3, nearest 2x upsample folded into its consumer: the upsample writes the leading channels of a concat buffer that exactly one
// 1x1 conv reads (YOLO necks: Upsample -> Concat -> C2f.cv1); that conv then fetches those channels from the half-resolution tensor itself
// and the upsample launch (and its 4x larger copy of the tensor) disappears
void fold_upsamples(adas_engine* e, const Uses& u) {
    if (!(prec_is16(e->prec) || e->prec == PREC_X3) || env_on("ADAS_NO_UPSAMPLE_FOLD")) return;
    for (int ui = 0; ui < u.n_ops(); ++ui) {
        const FileOp& up = u.op(ui);
        if (up.type != OP_UPSAMPLE2 || e->ops[ui].skip || up.out_coff != 0 || (up.out_c & 31)) continue;
        // readers of the upsampled channel range (another slice of the same concat buffer may have its own readers)
        const Uses::Readers r = u.readers(up.out_buf, ui, up.out_coff, up.out_c);
        if (r.count != 1 || u.is_output(up.out_buf) || r.last <= ui || u.aliased(up.out_buf)) continue;
        const FileOp& c = u.op(r.last);
        if (c.type != OP_CONV || c.kh != 1 || c.kw != 1 || c.stride != 1 || c.pad != 0 || c.res_mode != RES_NONE || c.n_in != 1 || c.in_coff[0] != 0 ||
            c.in_c[0] <= up.out_c || e->ops[r.last].skip)
            continue;
        // only conv_pw reads ConvArgs::up: fold when the reader is PLANNED onto it (ADAS_NO_PW=1 plans it elsewhere)
        if (plan_conv(e->prec, 1, 1, 1, 0, e->max_batch, RES_NONE, in_view(e, c), out_view(e, c)).kernel != CONV_PW) continue;
        if (u.written_between(up.in_buf[0], ui, r.last)) continue;   // the low-resolution source is rewritten between the upsample and the conv
        e->ops[r.last].up_src = ui;
        e->ops[ui].skip = true;
    }
}

// ---- pass 4, three max-pools in one launch (sppf_pool3): SPPF's chained 5x5 s1 p2 pools, each reading the one before, and SPP's 5x5, 9x9
// and 13x13 stride-1 pools of ONE tensor (YOLOv7's SPPCSPC, YOLOv3/v4).  Stride-1 max-pools with -inf padding compose exactly (a 9x9 window
// clipped to the image = the 5x5 max of 5x5 maxima), so SPP's three are the chain's three outputs -- bit-identical, and the 81 / 169
// sequential loads per output of the generic kernel go away
void fuse_pool_chains(adas_engine* e) {
    if (env_on("ADAS_NO_POOL_FUSE")) return;
    auto isk = [](const FileOp& q, uint32_t k) { return q.type == OP_MAXPOOL && q.kh == k && q.stride == 1 && q.pad == k / 2 && q.n_in == 1; };
    auto same_in = [](const FileOp& a, const FileOp& b) { return a.in_buf[0] == b.in_buf[0] && a.in_coff[0] == b.in_coff[0] && a.in_c[0] == b.in_c[0]; };
    for (int spp = 0; spp < 2; ++spp)
        for (size_t i = 0; i + 2 < e->ops.size(); ++i) {
            const FileOp &p0 = e->ops[i].f, &p1 = e->ops[i + 1].f, &p2 = e->ops[i + 2].f;
            if (spp ? !isk(p0, 5) || !isk(p1, 9) || !isk(p2, 13) || !same_in(p0, p1) || !same_in(p0, p2) || e->ops[i].skip || e->ops[i + 1].skip || e->ops[i + 2].skip
                    : !isk(p0, 5) || !isk(p1, 5) || !isk(p2, 5) || !feeds(p0, p1) || !feeds(p1, p2) || e->ops[i].skip)
                continue;
            const TView outs[3] = {out_view(e, p0), out_view(e, p1), out_view(e, p2)};
            if (!sppf_pool3_applicable(e->prec, in_view(e, p0), outs)) continue;
            e->ops[i].pool3[0] = (int)i + 1;
            e->ops[i].pool3[1] = (int)i + 2;
            e->ops[i + 1].skip = e->ops[i + 2].skip = true;
            i += 2;
        }
}

// ---- pass 5, 3x3 -> 3x3 pair fusion (conv_pair.hip): conv A's output feeds only conv B (the Bottleneck of YOLOv8's C2f blocks)
void fuse_pairs(adas_engine* e, const Uses& u) {
    for (int ai = 0; ai + 1 < u.n_ops(); ++ai) {
        const FileOp& qa = u.op(ai);
        if (qa.type != OP_CONV || e->ops[ai].skip || e->ops[ai].kernel == CONV_STEM) continue;   // (skip: also the B of an earlier pair)
        const Uses::Readers r = u.readers(qa.out_buf, ai);
        const int bi = r.last;
        if (r.count != 1 || u.is_output(qa.out_buf) || bi <= ai || u.aliased(qa.out_buf)) continue;
        const FileOp& qb = u.op(bi);
        if (qb.type != OP_CONV || e->ops[bi].skip || qb.n_in != 1 || !feeds(qa, qb)) continue;
        // nothing between A and B writes A's input or B's output region's buffer in a way the fusion would reorder
        if (u.written_between(qa.in_buf[0], ai, bi) || u.written_between(qb.out_buf, ai, bi)) continue;
        const TView x = in_view(e, qa), t = out_view(e, qa), y = out_view(e, qb);
        const TView r2 = qb.res_mode != RES_NONE ? make_view(e, qb.res_buf, qb.res_coff, qb.out_c) : y;
        // the pair writes y while other workgroups still read x halos: y must not overlap x (same memory, intersecting channel ranges)
        if (y.p == x.p && y.coff < x.coff + x.c && x.coff < y.coff + y.c) continue;
        if (!pair_applicable(e->prec, qa.kh, qa.kw, qa.stride, qa.pad, qa.act, qa.res_mode, x, t, qb.kh, qb.kw, qb.stride, qb.pad, qb.act, qb.res_mode, y, r2) &&
            !pair_x3_candidate(e->prec, qa.kh, qa.kw, qa.stride, qa.pad, qa.act, qa.res_mode, x, t, qb.kh, qb.kw, qb.stride, qb.pad, qb.act, qb.res_mode, y))
            continue;
        e->ops[ai].pair_b = bi;
        e->ops[bi].skip = true;
    }
}

// The 1x1 convs behind a Detect op's inputs, when each feeds only the decode: what both Detect fusions start from.  `accepts(k, conv)`:
// the fusion's own conditions on the conv behind input k.
template <class F>
bool detect_sources(const adas_engine* e, const Uses& u, int di, int n, int* src, F accepts) {
    const FileOp& dq = u.op(di);
    for (int k = 0; k < n; ++k) {
        src[k] = u.producer(dq.in_buf[k], dq.in_coff[k], dq.in_c[k], di);
        if (src[k] < 0 || !accepts(k, e->ops[src[k]])) return false;
        const int logits = u.op(src[k]).out_buf;   // nobody else reads them
        if (u.readers(logits, di).count != 0 || u.is_output(logits) || u.aliased(logits)) return false;
    }
    return true;
}

// ---- pass 6, v5-layout Detect fusion (aux_kernels.hip detect_v5_fused_kernel): the per-level 1x1 convs feed only the decode; decided
// before the weight layout because the fused launch wants per-anchor MFMA fragments (CONV_DET5)
void fuse_detect_v5(adas_engine* e, const Uses& u) {
    for (int di = 0; di < u.n_ops(); ++di) {
        const FileOp& dq = u.op(di);
        if (dq.type != OP_DETECT_V5 || dq.n_in != 3) continue;
        int src[3];
        if (!detect_sources(e, u, di, 3, src, [&](int, const EngOp& c) {
                const FileOp& q = c.f;
                return q.kh == 1 && q.kw == 1 && q.stride == 1 && q.pad == 0 && q.act == ACT_NONE && q.res_mode == RES_NONE && q.n_in == 1 && !c.skip &&
                       det5_applicable(e->prec, (int)dq.params[0], in_view(e, q), out_view(e, q));
            }))
            continue;
        for (int k = 0; k < 3; ++k) {
            e->ops[di].det_src[k] = src[k];
            e->ops[src[k]].skip = true;
        }
    }
}

// ---- pass 7, whole-C2f fusion (conv_c2f.hip): cv1 1x1 -> [split] -> fused 3x3 pair with shortcut -> cv2 1x1 over the concat, when the
// concat buffer has no other reader: one launch, the concat is never written (YOLOv8n / YOLOv10n model.2)
void fuse_c2f(adas_engine* e, const Uses& u) {
    for (int ai = 0; ai < u.n_ops(); ++ai) {
        const int bi = e->ops[ai].pair_b;
        if (bi < 0) continue;
        const FileOp &qa = u.op(ai), &qb = u.op(bi);
        const int cat = qa.in_buf[0];
        if (qa.in_c[0] != 16 || qb.out_buf != cat || qb.out_coff != qa.in_coff[0] + 16 || qb.res_mode != RES_AFTER_ACT || qa.in_coff[0] < 16 || u.aliased(cat)) continue;
        if (qb.res_buf != cat || qb.res_coff != qa.in_coff[0]) continue;   // conv B's shortcut must be the y1 slice conv A reads (the fused kernel adds THAT)
        int c1 = -1, c2 = -1;
        for (int j = 0; j < u.n_ops(); ++j) {
            const FileOp& q = u.op(j);
            if (q.type != OP_CONV || q.kh != 1 || q.kw != 1 || q.stride != 1 || q.pad != 0 || q.act != ACT_SILU || q.res_mode != RES_NONE || q.n_in != 1 ||
                e->ops[j].skip)
                continue;
            if (j < ai && q.out_buf == cat && q.out_coff == qa.in_coff[0] - 16 && q.out_c == 32 && q.in_c[0] == 32 && e->ops[j].up_src < 0) c1 = j;
            if (j > bi && q.in_buf[0] == cat && q.in_coff[0] == qa.in_coff[0] - 16 && q.in_c[0] == 48 && q.out_c == 32) c2 = j;
        }
        if (c1 < 0 || c2 < 0 || u.readers(cat).count != 3 || u.is_output(cat)) continue;   // readers: conv A, conv B's shortcut, cv2
        bool sole_writers = true;   // nothing else writes into the concat buffer
        for (int j = 0; j < u.n_ops(); ++j) sole_writers = sole_writers && !(u.op(j).out_buf == cat && j != c1 && j != bi);
        if (!sole_writers) continue;
        const FileOp &q1 = u.op(c1), &q2 = u.op(c2);
        // the fused launch runs cv2 at cv1's position: nothing between cv1 and cv2 other than conv A / conv B may touch cv2's output buffer or
        // rewrite the block input, and cv2's output must not overlap the input whose halos other workgroups are still reading
        bool safe = !(q2.out_buf == q1.in_buf[0] && q2.out_coff < q1.in_coff[0] + q1.in_c[0] && q1.in_coff[0] < q2.out_coff + q2.out_c);
        for (int j = c1 + 1; j < c2 && safe; ++j)
            safe = j == ai || j == bi || !(u.op(j).out_buf == q2.out_buf || u.op(j).out_buf == q1.in_buf[0] || Uses::reads(u.op(j), q2.out_buf));
        if (!safe) continue;
        // conv_c2f.hip / conv_c2f_x3.hip address the input with 31-bit byte offsets (2 / 4 bytes per element): decided here, at max_batch, so
        // the engine never records a fusion its launcher refuses at run time
        const EngBuf& xb = e->bufs[q1.in_buf[0]];
        if ((double)e->max_batch * xb.h * xb.w * xb.c * (e->prec == PREC_X3 ? 4.0 : 2.0) >= 2147483648.0) continue;
        const TView vx = in_view(e, q1), v01 = out_view(e, q1), vy1 = in_view(e, qa), vy2 = out_view(e, qb), vcat = in_view(e, q2), vout = out_view(e, q2);
        if (!c2f16_applicable(e->prec, vx, v01, vy1, vy2, vcat, vout) && !c2f16_x3_applicable(e->prec, vx, v01, vy1, vy2, vcat, vout)) continue;
        e->ops[c1].c2f[0] = ai; e->ops[c1].c2f[1] = bi; e->ops[c1].c2f[2] = c2;
        e->ops[ai].skip = true;   // (conv B is skipped already: the pair launch is replaced as a whole)
        e->ops[c2].skip = true;
    }
}

// ---- pass 8, split precision: a pair exists only inside a fused C2f block (conv_c2f_x3.hip) -- release the others
void release_x3_pairs(adas_engine* e) {
    if (e->prec != PREC_X3) return;
    for (auto& a : e->ops) {
        if (a.pair_b < 0 || a.skip) continue;      // (skip: absorbed into a C2f launch above)
        e->ops[a.pair_b].skip = false;
        a.pair_b = -1;
    }
}

struct Arena {   // the weight arena's bump allocator: every piece starts on a 256-byte boundary
    size_t total = 0;
    size_t take(size_t bytes) {
        const size_t off = total;
        total += (bytes + 255) & ~(size_t)255;
        return off;
    }
};

// ---- pass 9, the weight arena: each conv's packing (its kernel class, fixed for the engine's life) and where every op's weights go
int layout_arena(adas_engine* e, const char* label) {
    const int prec = e->prec;
    const size_t esz = (size_t)prec_esize(prec);
    std::vector<int> fused(e->ops.size(), -1);   // the packing a fusion fixes for a conv: both convs of a pair, cv1 / cv2 of a C2f block, a v5 Detect's sources
    for (auto& op : e->ops)
        if (op.pair_b >= 0) fused[&op - e->ops.data()] = fused[op.pair_b] = CONV_PAIR;
    for (auto& op : e->ops)
        if (op.c2f[0] >= 0) fused[&op - e->ops.data()] = fused[op.c2f[2]] = CONV_C2F_PW;
    for (auto& op : e->ops)
        for (int k = 0; k < 3 && op.f.type == OP_DETECT_V5; ++k)
            if (op.det_src[k] >= 0) fused[op.det_src[k]] = CONV_DET5;
    Arena arena;
    for (auto& op : e->ops) {
        const FileOp& o = op.f;
        if (o.type == OP_CONV) {
            const int cin = o.in_c[0], cout = o.out_c;
            const bool stem = op.kernel == CONV_STEM, stem2 = op.kernel == CONV_STEM2;
            op.k = o.kh * o.kw * cin;
            op.cout_pad = (cout + 127) / 128 * 128;
            size_t w_bytes;
            if (stem || stem2) {
                op.kpad = stem ? 32 * o.kh : 160;
                op.cin_pad = stem ? 4 : 16;
                w_bytes = stem ? (prec == PREC_X3 ? stem_x3_weight_bytes(o.kh, o.out_c) : stem_weight_bytes(o.kh, o.out_c))
                               : (prec == PREC_X3 ? stem2_x3_weight_bytes() : stem2_weight_bytes());
            } else {
                const TView in = in_view(e, o), out = out_view(e, o);
                const ConvPlan pl = plan_conv(prec, o.kh, o.kw, o.stride, o.pad, e->max_batch, o.res_mode, in, out);
                ADAS_REQUIRE(pl.kernel != CONV_FC || o.res_mode == RES_NONE, ADAS_ERR_FORMAT, "[%s]: layer %s: a Linear layer cannot carry a residual", label,
                             op.name.c_str());
                // few tiles at this engine's max_batch: narrower channel blocks (fixes the packing: decided here)
                if (pl.kernel == CONV_HALO) op.halo_bn = plan_halo_bn(e->max_batch, (int)o.stride, in, out);
                op.kpad = pl.kpad;
                op.cin_pad = pl.cin_pad;
                const int fixed = fused[&op - e->ops.data()];
                op.kernel = fixed >= 0 ? fixed : pl.kernel;   // pair / C2f fragments fit the plan's allocation (<= 18 KB; 2 / 4 KB inside 8 / 16 KB)
                w_bytes = (size_t)op.cout_pad * op.kpad * esz;
                if (fixed == CONV_DET5) w_bytes = det5_weight_bytes(cout / 3, cin);   // per-anchor fragments: 3 x 96 rows, more than the plan's 256
                else {
                    if (wants_x3h8_packing(prec, pl.kernel, o.kh, o.kw, o.stride, o.pad, o.res_mode, in, out)) {
                        op.has_x3h8 = true;   // the batch decides at launch which of the two packings runs
                        op.x3h8_w_off = arena.take(halo8_x3_weight_bytes(cout, cin));
                    }
                    if (op.ds_user >= 0) op.ds_w_off = arena.take((size_t)cout * cin * esz);   // second copy of the projection weights, as per-step tiles
                }
            }
            op.w_off = arena.take(w_bytes);
            op.b_off = arena.take((size_t)op.cout_pad * 4);
        } else if (o.type == OP_LAYERNORM || o.type == OP_DWCONV || o.type == OP_SE_GATE) {
            op.w_off = arena.take((size_t)o.w_elems * 4);
            op.b_off = arena.take((size_t)o.b_elems * 4);
        } else if (o.type == OP_DETECT_V5) {
            op.w_off = arena.take(18 * sizeof(float));   // the anchors
        }
    }
    e->weight_bytes = arena.total;
    return ADAS_OK;
}

// ---- pass 10, v8 Detect fusion (aux_kernels.hip detect_v8_fused_kernel; split precision: detect_v8_fused_x3_kernel): the last 1x1 convs
// of both head branches feed only the decode.  Reads kernel / kpad / cout_pad: after the layout
void fuse_detect_v8(adas_engine* e, const Uses& u) {
    if (!(prec_is16(e->prec) || e->prec == PREC_X3) || env_on("ADAS_NO_DETECT_FUSE")) return;
    for (int di = 0; di < u.n_ops(); ++di) {
        EngOp& dop = e->ops[di];
        if (dop.f.type != OP_DETECT_V8 || dop.f.n_in != 6) continue;
        int src[6];
        bool ok = detect_sources(e, u, di, 6, src, [&](int k, const EngOp& c) {
            const FileOp& q = c.f;
            return q.kh == 1 && q.kw == 1 && q.stride == 1 && q.act == ACT_NONE && q.res_mode == RES_NONE && c.kernel == CONV_PW && !c.skip &&
                   e->bufs[q.out_buf].f32 && !e->bufs[q.in_buf[0]].f32 && (q.in_c[0] & 7) == 0 && q.out_c == (k % 2 == 0 ? 64u : (uint32_t)dop.f.params[0]);
        });
        for (int l = 1; l < 3 && ok; ++l)  // one hidden width per branch
            ok = e->ops[src[2 * l]].f.in_c[0] == e->ops[src[0]].f.in_c[0] && e->ops[src[2 * l + 1]].f.in_c[0] == e->ops[src[1]].f.in_c[0];
        if (ok) {  // the fused launch keeps both weight matrices in LDS: leave very wide heads / class counts to the separate kernels
            const size_t ksb = (e->ops[src[0]].f.in_c[0] + 31) / 32, ksc = (e->ops[src[1]].f.in_c[0] + 31) / 32;
            const size_t ntc = ((size_t)dop.f.params[0] + 15) / 16;
            const size_t frag = e->prec == PREC_X3 ? 2048 : 1024;   // a 16x32 weight fragment: halves, or (hi, lo) half pairs
            if (ksc > 12 || (4 * ksb + ntc * ksc) * frag + (64 + ntc * 16) * 4 > 150 * 1024) ok = false;
            if (e->prec == PREC_X3)   // the fused kernel indexes conv_pw_x3's packing: [16-feature tile][kpad / 32]
                for (int k = 0; k < 6 && ok; ++k) {
                    const EngOp& c = e->ops[src[k]];
                    ok = c.kpad == e->ops[src[k % 2]].kpad && (size_t)c.kpad >= (k % 2 ? ksc : ksb) * 32 && (c.kpad & 31) == 0 &&
                         (size_t)c.cout_pad >= (k % 2 ? ntc * 16 : 64);
                }
            if (e->prec == PREC_X3 && ok && (size_t)e->ops[src[1]].kpad / 32 > 12) ok = false;
        }
        if (!ok) continue;
        for (int k = 0; k < 6; ++k) {
            dop.det_src[k] = src[k];
            e->ops[src[k]].skip = true;
        }
    }
}

// ---- phase 3: the passes in the order they depend on each other (a pass skips what an earlier one took; the C2f fusion builds on the
// pairs; the layout packs for the fusions decided before it, and the v8 Detect fusion reads the layout)
int plan_engine(adas_engine* e, const char* label) {
    Placeholders ids(e);
    const Uses u{e};
    fuse_stem(e, u);
    link_shortcuts(e, u);
    fold_upsamples(e, u);
    fuse_pool_chains(e);
    fuse_pairs(e, u);
    fuse_detect_v5(e, u);
    fuse_c2f(e, u);
    release_x3_pairs(e);
    const int rc = layout_arena(e, label);
    if (rc == ADAS_OK) fuse_detect_v8(e, u);
    return rc;
}

// ---- phase 4 ----
int upload_bias(adas_engine* e, const EngOp& op, Source& src) {   // [cout_pad] fp32, the tail zero
    std::vector<float> b(op.cout_pad, 0.f);
    if (op.f.b_elems > b.size() || !src.read_at(e->hdr.weights_off + op.f.b_off, b.data(), op.f.b_elems * 4)) return ADAS_ERR_FORMAT;
    return hipMemcpy((unsigned char*)e->d_weights + op.b_off, b.data(), b.size() * 4, hipMemcpyHostToDevice) == hipSuccess ? ADAS_OK : ADAS_ERR_HIP;
}

// One op's weights: the fp32 blob goes through the staging buffers (h_stage, d_stage: room for the largest blob) and is packed on the device
int upload_op(adas_engine* e, const EngOp& op, Source& src, std::vector<float>& h_stage, float* d_stage) {
    const FileOp& o = op.f;
    const int prec = e->prec;
    unsigned char* base = (unsigned char*)e->d_weights;
    auto read_blob = [&](uint64_t off, uint64_t elems, float* dst) { return src.read_at(e->hdr.weights_off + off, dst, elems * 4); };
    auto to_device = [](void* dst, const void* from, size_t bytes) { return hipMemcpy(dst, from, bytes, hipMemcpyHostToDevice) == hipSuccess; };
    if (o.type == OP_CONV) {
        if (o.w_elems != (uint64_t)o.out_c * op.k || !read_blob(o.w_off, o.w_elems, h_stage.data())) return ADAS_ERR_FORMAT;
        if (!to_device(d_stage, h_stage.data(), o.w_elems * 4)) return ADAS_ERR_HIP;
        if (op.kernel == CONV_STEM || op.kernel == CONV_STEM2) {   // packed on the host
            std::vector<uint16_t> frag((op.kernel == CONV_STEM2 ? (prec == PREC_X3 ? stem2_x3_weight_bytes() : stem2_weight_bytes())
                                        : prec == PREC_X3       ? stem_x3_weight_bytes(o.kh, o.out_c)
                                                                : stem_weight_bytes(o.kh, o.out_c)) / 2);
            if (op.kernel == CONV_STEM2 && prec == PREC_X3) stem2_x3_pack_weights(h_stage.data(), frag.data());
            else if (op.kernel == CONV_STEM2) stem2_pack_weights(h_stage.data(), frag.data(), prec);
            else if (prec == PREC_X3) stem_x3_pack_weights(h_stage.data(), o.out_c, o.kh, o.kw, o.in_c[0], e->hdr.in_c, frag.data());
            else stem_pack_weights(h_stage.data(), o.out_c, o.kh, o.kw, o.in_c[0], e->hdr.in_c, frag.data(), prec);
            if (!to_device(base + op.w_off, frag.data(), frag.size() * 2)) return ADAS_ERR_HIP;
            return upload_bias(e, op, src);
        }
        hipError_t pe = op.kernel == CONV_DET5 ? launch_pack_weights_det5(d_stage, base + op.w_off, o.out_c / 3, o.in_c[0], prec, 0)
                        : op.kernel == CONV_C2F_PW ? (prec == PREC_X3 ? launch_pack_weights_c2f_pw_x3(d_stage, base + op.w_off, o.out_c, o.in_c[0], 0)
                                                                       : launch_pack_weights_c2f_pw(d_stage, base + op.w_off, o.out_c, o.in_c[0], prec, 0))
                        : op.kernel == CONV_PAIR ? (prec == PREC_X3 ? launch_pack_weights_pair16_x3(d_stage, base + op.w_off, 0)
                                                                     : launch_pack_weights_pair(d_stage, base + op.w_off, o.out_c, prec, 0))
                        : (op.kernel == CONV_FC || op.kernel == CONV_PW)
                            ? launch_pack_weights_fc(d_stage, base + op.w_off, o.out_c, op.cout_pad, o.in_c[0], op.kpad, prec, 0)
                            : op.kernel == CONV_HALO
                            ? launch_pack_weights_halo(d_stage, base + op.w_off, o.out_c, op.cout_pad, o.in_c[0], op.cin_pad, prec, 0, op.halo_bn)
                            : launch_pack_weights(d_stage, base + op.w_off, o.out_c, op.cout_pad, o.kh * o.kw, o.in_c[0], op.cin_pad, op.kpad, prec, 0);
        if (pe == hipSuccess && op.has_x3h8) pe = launch_pack_weights_h8x3(d_stage, base + op.x3h8_w_off, o.out_c, o.in_c[0], 0);
        if (pe == hipSuccess && op.ds_user >= 0) pe = launch_pack_weights_ds(d_stage, base + op.ds_w_off, o.out_c, o.in_c[0], prec, 0);
        if (pe != hipSuccess || hipDeviceSynchronize() != hipSuccess) return ADAS_ERR_HIP;   // (the next op reuses d_stage)
        return upload_bias(e, op, src);
    }
    if (o.type == OP_LAYERNORM || o.type == OP_SE_GATE || o.type == OP_DWCONV) {   // fp32 in every precision, both blobs as they are ...
        if (!read_blob(o.w_off, o.w_elems, h_stage.data())) return ADAS_ERR_FORMAT;
        std::vector<float> wt;
        if (o.type == OP_DWCONV) {   // ... but for the depth-wise taps: container [C][kh][kw] -> device [kh*kw][C] (36..6272 floats per layer)
            const size_t C_ = o.out_c, T_ = (size_t)o.kh * o.kw;
            wt.resize(C_ * T_);
            for (size_t c = 0; c < C_; ++c)
                for (size_t t = 0; t < T_; ++t) wt[t * C_ + c] = h_stage[c * T_ + t];
        }
        if (!to_device(base + op.w_off, wt.empty() ? h_stage.data() : wt.data(), o.w_elems * 4)) return ADAS_ERR_HIP;
        if (!read_blob(o.b_off, o.b_elems, h_stage.data())) return ADAS_ERR_FORMAT;
        return to_device(base + op.b_off, h_stage.data(), o.b_elems * 4) ? ADAS_OK : ADAS_ERR_HIP;
    }
    if (o.type == OP_DETECT_V5) {
        float anc[18];
        if (o.w_elems != 18 || !read_blob(o.w_off, 18, anc)) return ADAS_ERR_FORMAT;
        return to_device(base + op.w_off, anc, sizeof(anc)) ? ADAS_OK : ADAS_ERR_HIP;
    }
    return ADAS_OK;
}

int allocate_and_upload(adas_engine* e, Source& src, const char* label) {
    for (auto& b : e->bufs) {
        if (b.alias_of >= 0) continue;
        const size_t bytes = (size_t)e->max_batch * b.h * b.w * b.c * elem_size(e, b);
        if (hipMalloc(&b.d, bytes + 256) != hipSuccess) return hip_fail(hipGetLastError(), "hipMalloc(activation buffer)", __FILE__, __LINE__);
        (void)hipMemset(b.d, 0, bytes + 256);
        e->act_bytes += bytes;
    }
    for (auto& b : e->bufs)
        if (b.alias_of >= 0) b.d = e->bufs[b.alias_of].d;
    // ---- weights: stream the fp32 blobs through a staging buffer, pack on the device
    if (hipMalloc(&e->d_weights, e->weight_bytes + 256) != hipSuccess) return hip_fail(hipGetLastError(), "hipMalloc(weights)", __FILE__, __LINE__);
    (void)hipMemset(e->d_weights, 0, e->weight_bytes + 256);
    size_t max_w = 0;
    for (auto& op : e->ops) {
        max_w = op.f.w_elems > max_w ? (size_t)op.f.w_elems : max_w;
        max_w = op.f.b_elems > max_w ? (size_t)op.f.b_elems : max_w;   // layernorm / squeeze-and-excitation stage their second blob too
    }
    ADAS_REQUIRE(max_w <= src.size / 4, ADAS_ERR_FORMAT, "[%s]: failed while loading weights (bad blob)", label);
    float* d_stage = nullptr;
    std::vector<float> h_stage(max_w ? max_w : 1);
    if (hipMalloc((void**)&d_stage, max_w * 4 + 256) != hipSuccess) return hip_fail(hipGetLastError(), "hipMalloc(weight staging)", __FILE__, __LINE__);
    int rc = ADAS_OK;
    for (size_t i = 0; i < e->ops.size() && rc == ADAS_OK; ++i) rc = upload_op(e, e->ops[i], src, h_stage, d_stage);
    (void)hipFree(d_stage);
    ADAS_REQUIRE(rc == ADAS_OK, rc, "[%s]: failed while loading weights (%s)", label, rc == ADAS_ERR_HIP ? hipGetErrorString(hipGetLastError()) : "bad blob");
    const size_t in_bytes = (size_t)e->max_batch * e->hdr.in_c * e->hdr.in_h * e->hdr.in_w * 4;
    if (hipMalloc((void**)&e->d_input, in_bytes) != hipSuccess) return hip_fail(hipGetLastError(), "hipMalloc(input staging)", __FILE__, __LINE__);
    // the schedule of the engine's own batch size and its grouped / multi-layer launch tables are built now, not on the first forward
    // (device allocations and synchronous copies do not belong on the hot path; other batch sizes are prepared on first use, engine_forward)
    return engine_prepare(e, e->max_batch) == ADAS_OK ? ADAS_OK : ADAS_ERR_HIP;
}

bool known_precision(int p) { return p == ADAS_PREC_BF16 || p == ADAS_PREC_FP32 || p == ADAS_PREC_FP16 || p == ADAS_PREC_FP16X3; }

// one row of ADAS_PLAN_COLS per op, the columns in the order include/adas_hip.h documents
int write_plan_rows(const adas_engine* e, int64_t* rows, int rows_cap, int32_t* n_ops, uint64_t* weight_bytes) {
    if (n_ops) *n_ops = (int32_t)e->ops.size();
    if (weight_bytes) *weight_bytes = e->weight_bytes;
    if (!rows) return ADAS_OK;
    ADAS_REQUIRE(rows_cap >= (int)e->ops.size(), ADAS_ERR_CAPACITY, "engine plan: %zu layers, room for %d", e->ops.size(), rows_cap);
    for (const EngOp& op : e->ops) {
        int64_t* r = rows + (size_t)(&op - e->ops.data()) * ADAS_PLAN_COLS;
        int c = 0;
        r[c++] = op.kernel; r[c++] = op.skip; r[c++] = op.fuse_pool; r[c++] = op.fuse_conv2; r[c++] = op.ds_src; r[c++] = op.ds_user; r[c++] = op.up_src;
        for (int v : op.pool3) r[c++] = v;
        r[c++] = op.pair_b;
        for (int v : op.c2f) r[c++] = v;
        for (int v : op.det_src) r[c++] = v;
        r[c++] = op.halo_bn; r[c++] = op.has_x3h8; r[c++] = op.k; r[c++] = op.kpad; r[c++] = op.cin_pad; r[c++] = op.cout_pad;
        r[c++] = (int64_t)op.w_off; r[c++] = (int64_t)op.b_off; r[c++] = (int64_t)op.ds_w_off; r[c++] = (int64_t)op.x3h8_w_off;
        static_assert(ADAS_PLAN_COLS == 29, "plan row layout (include/adas_hip.h)");
    }
    return ADAS_OK;
}

}  // namespace

bool adas::wants_x3h8_packing(int precision, int kernel, int kh, int kw, int stride, int pad, int res_mode, const TView& in, const TView& out) {
    return precision == PREC_X3 && kernel != CONV_PW && kernel != CONV_FC &&
           (halo8_x3_shape_ok(kh, kw, stride, pad, in, out) || halo_s2p_x3_shape_ok(kh, kw, stride, pad, res_mode, in, out));
}

extern "C" {

int adas_engine_create(const char* model_path, int precision, int max_batch, adas_engine** out) {
    ADAS_REQUIRE(model_path && out && max_batch > 0, ADAS_ERR_INVALID, "adas_engine_create: bad argument");
    ADAS_REQUIRE(known_precision(precision), ADAS_ERR_INVALID, "unknown precision %d", precision);
    Source src;
    // coreEngine.py:12-13
    ADAS_REQUIRE(src.open(model_path), ADAS_ERR_IO, "The model path [%s] can't not found! (%s)", model_path, strerror(errno));
    EnginePtr e;
    int rc = read_container(src, model_path, true, precision, max_batch, e);
    if (rc == ADAS_OK) rc = validate_container(e.get(), model_path);
    if (rc == ADAS_OK) rc = plan_engine(e.get(), model_path);
    if (rc == ADAS_OK) rc = allocate_and_upload(e.get(), src, model_path);
    if (rc == ADAS_OK) *out = e.release();
    return rc;
}

int adas_engine_plan(const adas_engine* e, int64_t* rows, int rows_cap, int32_t* n_ops, uint64_t* weight_bytes) {
    ADAS_REQUIRE(e, ADAS_ERR_INVALID, "null engine");
    return write_plan_rows(e, rows, rows_cap, n_ops, weight_bytes);
}

int adas_debug_engine_plan(const void* tables, size_t bytes, int precision, int max_batch, int64_t* rows, int rows_cap, int32_t* n_ops,
                           uint64_t* weight_bytes) {
    ADAS_REQUIRE(tables && max_batch > 0, ADAS_ERR_INVALID, "adas_debug_engine_plan: bad argument");
    ADAS_REQUIRE(known_precision(precision), ADAS_ERR_INVALID, "unknown precision %d", precision);
    Source src(tables, bytes);
    EnginePtr e;
    int rc = read_container(src, "tables", false, precision, max_batch, e);
    if (rc == ADAS_OK) rc = validate_container(e.get(), "tables");
    if (rc == ADAS_OK) rc = plan_engine(e.get(), "tables");
    if (rc == ADAS_OK) rc = write_plan_rows(e.get(), rows, rows_cap, n_ops, weight_bytes);
    return rc;
}

int adas_debug_engine_schedule(const void* tables, size_t bytes, int precision, int max_batch, int batch, int32_t* step_of, int32_t* role, char* labels,
                               int cap, int32_t* n_ops, int32_t* n_steps) {
    ADAS_REQUIRE(tables && max_batch > 0 && batch > 0 && batch <= max_batch, ADAS_ERR_INVALID, "adas_debug_engine_schedule: bad argument");
    ADAS_REQUIRE(known_precision(precision), ADAS_ERR_INVALID, "unknown precision %d", precision);
    Source src(tables, bytes);
    EnginePtr e;
    int rc = read_container(src, "tables", false, precision, max_batch, e);
    if (rc == ADAS_OK) rc = validate_container(e.get(), "tables");
    if (rc == ADAS_OK) rc = plan_engine(e.get(), "tables");
    if (rc != ADAS_OK) return rc;
    Placeholders ids(e.get());
    Schedule s = plan_schedule(e.get(), batch, true);
    rc = write_schedule_rows(e.get(), s, batch, step_of, role, labels, cap, n_ops, n_steps);
    free_schedule(&s);
    return rc;
}

}  // extern "C"
