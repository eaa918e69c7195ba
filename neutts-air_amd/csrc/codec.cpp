// codec.cpp -- NeuCodec decoder engine behind include/neutts_hip.h (ntts_codec_*).
//
// Replaces  self.codec.decode_code(codes[1,1,T]) -> wav[1,1,480*T]  (ref:neutts/neutts.py:288-291) for a batch
// of utterances: one non-autoregressive pass, all Linear/Conv1d/DFT work on the MFMA GEMM (gemm.h), the rest
// in kernels/codec.h.  Weights keep the parameter names of transformers' Xcodec2Model.
#include <ntts/dev.h>

#include <math.h>
#include <stdarg.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <numeric>
#include <string>
#include <utility>
#include <vector>

#include "../../include/neutts_hip.h"
#include "kernels/codec.h"
#include "kernels/gemm.h"
#include "wav_stream.h"

using namespace ntts;

static std::string g_codec_create_err;

struct ResW { float *g1, *b1, *cb1, *g2, *b2, *cb2; bf16_t *w1, *w2; };
struct CLayerW { float *ln1, *ln2; bf16_t *wqkv, *wo, *fc1, *fc2; };

struct ntts_codec {
    ntts_codec_config cfg{};
    int device = 0;
    hipStream_t stream = nullptr;      // where the passes run: the engine's own stream or one the caller lent (ntts_codec_set_stream)
    hipStream_t own_stream = nullptr;
    std::string err;
    int H = 0, I = 0, nq = 0, n_fft = 0, nb = 0, NS = 0, lds_spec = 0;
    long K3 = 0, max_rows = 0;
    bool finalized = false;
    int S = 1;                   // 3 with precision = high: every bf16 GEMM operand is a split row [hi | lo | hi] of 3 x its columns (codec.h put_op)
    int fmt = kOpF16;            // operand format the non-GEMM kernels write (codec.h put_op): kOpF16 (default) / kOpSplit (high) / kOpBf16
    std::map<std::string, std::vector<float>> host;            // staged fp32 tensors until finalize
    std::map<std::string, std::vector<int64_t>> shapes;
    std::vector<void*> allocs;
    // device weights
    float *wf = nullptr, *bf = nullptr, *embed_b = nullptr, *fn_w = nullptr, *fn_b = nullptr, *head_b = nullptr, *win2 = nullptr;
    bf16_t *embed_w = nullptr, *head_w = nullptr, *basis3 = nullptr;
    ResW res[4]{};
    std::vector<CLayerW> layers;
    // workspaces
    float *h = nullptr, *t1 = nullptr, *spec = nullptr, *frames = nullptr, *wav = nullptr;
    bf16_t *xa = nullptr, *xb = nullptr, *qkv = nullptr, *act = nullptr, *vt = nullptr, *s3 = nullptr;
    int* meta = nullptr;
    size_t meta_cap = 0;
    // page-locked staging ring of the meta block (as backbone.cpp upload_meta): the copy from a pageable vector needed a stream-wide
    // synchronisation, which on a LENT stream (an engine gang's lane with a whole decode phase queued) blocked the launching thread
    static constexpr int kMetaStages = 2;
    int* meta_host[kMetaStages] = {nullptr, nullptr};
    hipEvent_t meta_ev[kMetaStages] = {nullptr, nullptr};
    bool meta_used[kMetaStages] = {false, false};
    int meta_next = 0;
    size_t wav_cap = 0;
    hipEvent_t ev[2]{};
    hipEvent_t ev_in = nullptr;   // orders a pass behind the stream that produced its device-side codes
    hipEvent_t ev_done = nullptr; // behind the asynchronous hand-over of the most recent pass (what ntts_codec_sync waits for on a lent stream)
    bool have_done = false;
    bool have_time = false;
    bool gn_reg = true;          // GroupNorm with the utterance slice in registers when it fits (NTTS_CODEC_GN_REG=0: the two-pass kernel)
    // per-stage taps of the residual stream (ntts_codec_set_debug / ntts_codec_read_stage: the error-budget tests): fp32 [4][max_rows][H]
    float* tap = nullptr;
    std::vector<int> tap_off, tap_len;   // row offset / frames of every utterance of the most recent decode call
    bool attn_resident = true;   // utterances of up to 256 frames: attn_full_resident_kernel (NTTS_CODEC_ATTN_RESIDENT=0: the two-sweep paged kernel)
    // output stage (ntts_wav_format): one coefficient table per (rate, filter width) used so far, kept until destroy; the formatted buffer
    // is allocated with the first call that needs it, for the engine's whole workspace at that call's rate and element size
    struct WavTable { float* coef; int orig, nw, width, taps; };
    std::map<std::pair<int, int>, WavTable> wav_tables;
    // a device buffer of the stages behind overlap-add: allocated by the first call that needs it, grown by a later one (grow), freed with the engine
    template <typename T>
    struct Grown { T* p = nullptr; size_t cap = 0; };      // cap counts elements of T
    Grown<char> fbuf;
    // time stretch (ntts_codec_stretch / _decode_speed): the stretched 24 kHz waveforms and their frame positions, allocated with the first call
    // that needs them for twice the waveform workspace (speed 0.5 doubles a row); the fade table; events around the two kernels
    Grown<float> sbuf;
    Grown<int> spos;
    float* sfade = nullptr;
    hipEvent_t ev_s[3]{};
    bool have_stretch_time = false;
    // loudness (ntts_codec_normalize / _decode_loud): sub-block powers, the measure kernel's partial peaks and (L, peak, g) per row, allocated with
    // the first call that needs them; the K-weighting coefficients; events around the measure and the apply kernel
    Grown<double> lz;
    Grown<float> lpk;
    Grown<double> lres;
    double kw[7]{};
    hipEvent_t ev_l[4]{};
    bool have_loud_time = false;
};

static int cfail(ntts_codec* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf; else g_codec_create_err = buf;
    return code;
}
#define CHIP(c, call)                                                                                  \
    do {                                                                                               \
        hipError_t _s = (call);                                                                        \
        if (_s != hipSuccess) return cfail(c, _s == 2 ? NTTS_ENOMEM : NTTS_EHIP, "%s failed: %s", #call, hipGetErrorString(_s)); \
    } while (0)

extern "C" const char* ntts_codec_last_error(const ntts_codec* c) { return c ? c->err.c_str() : g_codec_create_err.c_str(); }

template <typename T>
static int dalloc(ntts_codec* c, T** p, size_t n) {
    void* v = nullptr;
    CHIP(c, hipMalloc(&v, n * sizeof(T)));
    c->allocs.push_back(v);
    *p = (T*)v;
    return NTTS_OK;
}

extern "C" void ntts_codec_destroy(ntts_codec* c) {
    if (!c) return;
    hipSetDevice(c->device);
    hipDeviceSynchronize();
    for (void* p : c->allocs) hipFree(p);
    if (c->tap) hipFree(c->tap);
    for (void* p : {(void*)c->fbuf.p, (void*)c->sbuf.p, (void*)c->spos.p, (void*)c->lz.p, (void*)c->lpk.p, (void*)c->lres.p})
        if (p) hipFree(p);
    for (auto& e : c->ev_s)
        if (e) hipEventDestroy(e);
    for (auto& e : c->ev_l)
        if (e) hipEventDestroy(e);
    for (auto& e : c->ev)
        if (e) hipEventDestroy(e);
    if (c->ev_in) hipEventDestroy(c->ev_in);
    if (c->ev_done) hipEventDestroy(c->ev_done);
    for (int i = 0; i < ntts_codec::kMetaStages; ++i) {
        if (c->meta_host[i]) hipHostFree(c->meta_host[i]);
        if (c->meta_ev[i]) hipEventDestroy(c->meta_ev[i]);
    }
    if (c->own_stream) hipStreamDestroy(c->own_stream);
    delete c;
}

extern "C" int ntts_codec_create(const ntts_codec_config* cf, int device, ntts_codec** out) {
    if (!cf || !out) return cfail(nullptr, NTTS_EINVAL, "null argument");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device || device < 0)
        return cfail(nullptr, NTTS_ENODEV, "no HIP device %d (found %d): this library has no CPU fallback", device, ndev);
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess || strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return cfail(nullptr, NTTS_ENODEV, "device %d is '%s', kernels are built for gfx950 only", device, prop.gcnArchName);
    if (cf->head_dim != 64 || cf->num_heads * 64 != cf->hidden_size) return cfail(nullptr, NTTS_EINVAL, "need head_dim 64 and heads*64 == hidden");
    if (cf->hidden_size % 64 || cf->intermediate_size % 64 || cf->hidden_size > 2048 || (cf->hidden_size / 32) > 256 || 256 % (cf->hidden_size / 32))
        return cfail(nullptr, NTTS_EINVAL, "unsupported hidden/intermediate size");
    if (cf->n_levels < 1 || cf->n_levels > 8 || cf->hop_length < 8 || (cf->hop_length % 8)) return cfail(nullptr, NTTS_EINVAL, "bad levels / hop");
    if (cf->max_frames < 1 || cf->max_rows < cf->max_frames + 2 * kPadRows) return cfail(nullptr, NTTS_EINVAL, "bad max_frames / max_rows");
    ntts_codec* c = new ntts_codec();
    c->cfg = *cf;
    c->device = device;
    c->H = cf->hidden_size; c->I = cf->intermediate_size; c->nq = cf->n_levels;
    c->n_fft = cf->hop_length * 4; c->nb = c->n_fft / 2 + 1; c->NS = c->n_fft + 2;
    c->lds_spec = (c->NS + 3) / 4 * 4;
    c->K3 = ((cf->precision == 0 ? 2L : 6L) * c->nb + 63) / 64 * 64;      // fp16: one term per (re, im) bin; bf16 engines: the hi / lo split, three terms
    c->max_rows = cf->max_rows;
    if (cf->precision < 0 || cf->precision > 2) { delete c; return cfail(nullptr, NTTS_EINVAL, "unknown codec precision %d (0 = fp16 operands, 1 = high: split bf16 operands, 2 = bf16 operands)", cf->precision); }
    c->S = cf->precision == 1 ? 3 : 1;
    c->fmt = cf->precision == 0 ? kOpF16 : cf->precision == 1 ? kOpSplit : kOpBf16;
    { const char* ev = getenv("NTTS_CODEC_ATTN_RESIDENT"); if (ev && ev[0] == '0') c->attn_resident = false; }
    { const char* ev = getenv("NTTS_CODEC_GN_REG"); if (ev && ev[0] == '0') c->gn_reg = false; }
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return cfail(nullptr, NTTS_EHIP, "stream creation failed");
    }
    c->stream = c->own_stream;
    hipEventCreate(&c->ev[0]); hipEventCreate(&c->ev[1]); hipEventCreate(&c->ev_in);
    hipEventCreateWithFlags(&c->ev_done, hipEventDisableTiming);
    const size_t R = c->max_rows, H = c->H;
    const int npages_max = (cf->max_frames + kPage - 1) / kPage;
    const size_t max_utts = R / (1 + 2 * kPadRows) + 1;
    int rc = NTTS_OK;
#define A(call) if (rc == NTTS_OK) rc = (call)
    const size_t S = c->S;        // (split operands: 3 x the columns)
    A(dalloc(c, &c->h, R * H)); A(dalloc(c, &c->t1, R * H)); A(dalloc(c, &c->xa, R * H * S)); A(dalloc(c, &c->xb, R * H * S));
    A(dalloc(c, &c->qkv, R * 3 * H)); A(dalloc(c, &c->act, R * c->I * S));
    A(dalloc(c, &c->vt, (R + (size_t)max_utts * kPage) * H));
    A(dalloc(c, &c->spec, R * c->lds_spec)); A(dalloc(c, &c->s3, R * c->K3)); A(dalloc(c, &c->frames, R * c->n_fft));
    c->wav_cap = R * cf->hop_length;
    A(dalloc(c, &c->wav, c->wav_cap));
    c->meta_cap = R + 3 * max_utts + 64;
    A(dalloc(c, &c->meta, c->meta_cap));
    for (int i = 0; i < ntts_codec::kMetaStages && rc == NTTS_OK; ++i)
        if (hipHostMalloc((void**)&c->meta_host[i], c->meta_cap * sizeof(int), hipHostMallocDefault) != hipSuccess ||
            hipEventCreateWithFlags(&c->meta_ev[i], hipEventDisableTiming) != hipSuccess) rc = cfail(nullptr, NTTS_ENOMEM, "page-locked meta staging");
    (void)npages_max;
    if (rc == NTTS_OK) {
        hipMemset(c->h, 0, R * H * 4); hipMemset(c->t1, 0, R * H * 4);
        hipMemset(c->xa, 0, R * H * S * 2); hipMemset(c->xb, 0, R * H * S * 2);
        hipMemset(c->qkv, 0, R * 3 * H * 2);
        hipDeviceSynchronize();
    } else {
        g_codec_create_err = c->err;
        ntts_codec_destroy(c);
        return rc;
    }
    *out = c;
    return NTTS_OK;
}

extern "C" int ntts_codec_load_tensor(ntts_codec* c, const char* name, const void* data, int dtype, const int64_t* shape,
                                      int ndim, int is_device) {
    if (!c || !name || !data || !shape || ndim < 1 || ndim > 3) return cfail(c, NTTS_EINVAL, "bad argument");
    if (c->finalized) return cfail(c, NTTS_ESTATE, "weights already finalised");
    if (dtype != NTTS_DT_F32 && dtype != NTTS_DT_BF16) return cfail(c, NTTS_EINVAL, "tensor '%s': dtype must be f32 or bf16", name);
    CHIP(c, hipSetDevice(c->device));
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
    const size_t esz = dtype == NTTS_DT_F32 ? 4 : 2;
    std::vector<unsigned char> raw(n * esz);
    if (is_device) CHIP(c, hipMemcpy(raw.data(), data, n * esz, hipMemcpyDeviceToHost));
    else memcpy(raw.data(), data, n * esz);
    std::vector<float> v(n);
    if (dtype == NTTS_DT_F32) memcpy(v.data(), raw.data(), n * 4);
    else
        for (size_t i = 0; i < n; ++i) {
            const uint32_t u = (uint32_t)((const uint16_t*)raw.data())[i] << 16;
            memcpy(&v[i], &u, 4);
        }
    c->host[name] = std::move(v);
    c->shapes[name] = std::vector<int64_t>(shape, shape + ndim);
    return NTTS_OK;
}

static bf16_t h_f2bf(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (bf16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (bf16_t)(u >> 16);
}
// float -> IEEE half, round-to-nearest-even (|f| <= 65504 checked by the caller)
static bf16_t h_f2h(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    const bf16_t sgn = (bf16_t)((u >> 16) & 0x8000u);
    const float a = fabsf(f);
    if (!(a == a)) return sgn | 0x7e00;
    if (a < 6.103515625e-05f) return sgn | (bf16_t)nearbyintf(ldexpf(a, 24));      // subnormal halves: multiples of 2^-24
    int ex;
    const float fr = frexpf(a, &ex);
    float mant = nearbyintf(ldexpf(fr, 11));
    int e = ex - 1 + 15;
    if (mant == 2048.0f) { mant = 1024.0f; e += 1; }
    if (e >= 31) return sgn | 0x7bff;
    return sgn | (bf16_t)((e << 10) | ((int)mant - 1024));
}
static float h_bf2f(bf16_t b) {
    const uint32_t u = (uint32_t)b << 16;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

struct Finalizer {
    ntts_codec* c;
    int rc = NTTS_OK;
    const std::vector<float>* get(const std::string& name, std::initializer_list<int64_t> shp) {
        auto it = c->host.find(name);
        if (it == c->host.end()) { rc = cfail(c, NTTS_ESTATE, "tensor '%s' not loaded", name.c_str()); return nullptr; }
        const auto& s = c->shapes[name];
        if (s.size() != shp.size() || !std::equal(s.begin(), s.end(), shp.begin())) {
            rc = cfail(c, NTTS_EINVAL, "tensor '%s': unexpected shape", name.c_str());
            return nullptr;
        }
        return &it->second;
    }
    float* up_f32(const std::vector<float>& v) {
        float* d = nullptr;
        if (dalloc(c, &d, v.size()) != NTTS_OK || hipMemcpy(d, v.data(), v.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { rc = NTTS_EHIP; return nullptr; }
        return d;
    }
    // a GEMM weight in the engine's 16-bit operand format: bf16, or IEEE half (precision = fp16: the values must fit its range)
    bf16_t* up_bf16(const std::vector<float>& v) {
        std::vector<bf16_t> b(v.size());
        if (c->fmt == kOpF16) {
            for (size_t i = 0; i < v.size(); ++i) {
                if (!(fabsf(v[i]) <= 65504.0f)) { rc = cfail(c, NTTS_EINVAL, "a GEMM weight of magnitude %g does not fit fp16: create the engine with precision = 1 (high) or 2 (bf16)", (double)v[i]); return nullptr; }
                b[i] = h_f2h(v[i]);
            }
        } else
        for (size_t i = 0; i < v.size(); ++i) b[i] = h_f2bf(v[i]);
        bf16_t* d = nullptr;
        if (dalloc(c, &d, b.size()) != NTTS_OK || hipMemcpy(d, b.data(), b.size() * 2, hipMemcpyHostToDevice) != hipSuccess) { rc = NTTS_EHIP; return nullptr; }
        return d;
    }
    // a GEMM weight [rows][K] whose X operand is made of segments of `seg` columns (the activation buffer's row width: K = seg for a
    // Linear, K = taps x seg for a conv over overlapping rows).  precision = high: every segment becomes [wh | wh | wl] (3 seg columns),
    // the counterpart of the split activation row [xh | xl | xh] (codec.h put_op): the K-loop forms xh wh + xl wh + xh wl
    bf16_t* op(const std::vector<float>& v, int64_t rows, int64_t K, int64_t seg) {
        if (c->S == 1) return up_bf16(v);
        std::vector<bf16_t> b((size_t)rows * 3 * K);
        for (int64_t r = 0; r < rows; ++r)
            for (int64_t s0 = 0; s0 < K; s0 += seg)
                for (int64_t i = 0; i < seg; ++i) {
                    const float w = v[(size_t)r * K + s0 + i];
                    const bf16_t hi = h_f2bf(w), lo = h_f2bf(w - h_bf2f(hi));
                    bf16_t* d = &b[(size_t)r * 3 * K + 3 * s0];
                    d[i] = hi; d[seg + i] = hi; d[2 * seg + i] = lo;
                }
        bf16_t* d = nullptr;
        if (dalloc(c, &d, b.size()) != NTTS_OK || hipMemcpy(d, b.data(), b.size() * 2, hipMemcpyHostToDevice) != hipSuccess) { rc = NTTS_EHIP; return nullptr; }
        return d;
    }
    float* vec(const std::string& name, int64_t n) {
        auto* v = get(name, {n});
        return v ? up_f32(*v) : nullptr;
    }
    bf16_t* mat(const std::string& name, int64_t r, int64_t k) {
        auto* v = get(name, {r, k});
        return v ? op(*v, r, k, k) : nullptr;
    }
    // Conv1d weight [Cout][Cin][k] -> GEMM weight [Cout][k][Cin]  (row of the overlapping-rows GEMM = k frames x Cin)
    bf16_t* conv(const std::string& name, int64_t co, int64_t ci, int64_t k) {
        auto* v = get(name, {co, ci, k});
        if (!v) return nullptr;
        std::vector<float> r((size_t)co * k * ci);
        for (int64_t o = 0; o < co; ++o)
            for (int64_t i = 0; i < ci; ++i)
                for (int64_t t = 0; t < k; ++t) r[((size_t)o * k + t) * ci + i] = (*v)[((size_t)o * ci + i) * k + t];
        return op(r, co, k * ci, ci);
    }
};

extern "C" int ntts_codec_finalize(ntts_codec* c) {
    if (!c) return NTTS_EINVAL;
    if (c->finalized) return NTTS_OK;
    CHIP(c, hipSetDevice(c->device));
    Finalizer f{c};
    const int64_t H = c->H, I = c->I, Q = c->cfg.quantization_dim, nq = c->nq, NS = c->NS;
    // ---- fold quantizer.project_out (nq -> Q) and decoder.fc (Q -> H): no nonlinearity in between
    {
        auto* pw = f.get("quantizer.project_out.weight", {Q, nq});
        auto* pb = f.get("quantizer.project_out.bias", {Q});
        auto* fw = f.get("decoder.fc.weight", {H, Q});
        auto* fb = f.get("decoder.fc.bias", {H});
        if (!pw || !pb || !fw || !fb) return f.rc;
        std::vector<float> wf((size_t)H * nq), bf(H);
        for (int64_t o = 0; o < H; ++o) {
            double b = (*fb)[o];
            std::vector<double> acc(nq, 0.0);
            for (int64_t q = 0; q < Q; ++q) {
                const double w = (*fw)[(size_t)o * Q + q];
                b += w * (*pb)[q];
                for (int64_t i = 0; i < nq; ++i) acc[i] += w * (*pw)[(size_t)q * nq + i];
            }
            bf[o] = (float)b;
            for (int64_t i = 0; i < nq; ++i) wf[(size_t)o * nq + i] = (float)acc[i];
        }
        c->wf = f.up_f32(wf); c->bf = f.up_f32(bf);
    }
    c->embed_w = f.conv("decoder.embed.weight", H, H, 7);
    c->embed_b = f.vec("decoder.embed.bias", H);
    const char* nets[2] = {"prior_net", "post_net"};
    for (int n = 0; n < 2; ++n)
        for (int b = 0; b < 2; ++b) {
            const std::string p = std::string("decoder.") + nets[n] + "." + std::to_string(b) + ".";
            ResW& r = c->res[n * 2 + b];
            r.g1 = f.vec(p + "norm1.weight", H); r.b1 = f.vec(p + "norm1.bias", H);
            r.w1 = f.conv(p + "conv1.weight", H, H, 3); r.cb1 = f.vec(p + "conv1.bias", H);
            r.g2 = f.vec(p + "norm2.weight", H); r.b2 = f.vec(p + "norm2.bias", H);
            r.w2 = f.conv(p + "conv2.weight", H, H, 3); r.cb2 = f.vec(p + "conv2.bias", H);
        }
    c->layers.resize(c->cfg.num_layers);
    for (int i = 0; i < c->cfg.num_layers && f.rc == NTTS_OK; ++i) {
        const std::string p = "decoder.layers." + std::to_string(i) + ".";
        CLayerW& L = c->layers[i];
        L.ln1 = f.vec(p + "input_layernorm.weight", H);
        L.ln2 = f.vec(p + "post_attention_layernorm.weight", H);
        auto* q = f.get(p + "self_attn.q_proj.weight", {H, H});
        auto* k = f.get(p + "self_attn.k_proj.weight", {H, H});
        auto* v = f.get(p + "self_attn.v_proj.weight", {H, H});
        if (!q || !k || !v) return f.rc;
        std::vector<float> qkv;
        qkv.reserve((size_t)3 * H * H);
        qkv.insert(qkv.end(), q->begin(), q->end()); qkv.insert(qkv.end(), k->begin(), k->end()); qkv.insert(qkv.end(), v->begin(), v->end());
        L.wqkv = f.op(qkv, 3 * H, H, H);
        L.wo = f.mat(p + "self_attn.o_proj.weight", H, H);
        L.fc1 = f.mat(p + "mlp.fc1.weight", I, H);
        L.fc2 = f.mat(p + "mlp.fc2.weight", H, I);
    }
    c->fn_w = f.vec("decoder.norm.weight", H); c->fn_b = f.vec("decoder.norm.bias", H);
    c->head_w = f.mat("decoder.head.linear.weight", NS, H);
    c->head_b = f.vec("decoder.head.linear.bias", NS);
    if (f.rc != NTTS_OK) return f.rc;
    // ---- windowed inverse real DFT as a GEMM operand, split hi/lo so bf16 MFMA reaches ~fp32 accuracy:
    //      frame[n] = hann[n]/N * ( Re0 + (-1)^n Re_{N/2} + 2 sum_k (Re_k cos(2 pi k n / N) - Im_k sin(2 pi k n / N)) )
    //      (torch.fft.irfft norm="backward" + window, hf:...modeling_xcodec2.py:776-777); row layout [B_hi | B_hi | B_lo].
    {
        const int N = c->n_fft, nb = c->nb;
        const long K3 = c->K3;
        std::vector<bf16_t> B((size_t)N * K3, 0);
        std::vector<float> w2(N);
        for (int n = 0; n < N; ++n) {
            const double win = 0.5 - 0.5 * cos(2.0 * M_PI * n / N);   // torch.hann_window (periodic)
            w2[n] = (float)(win * win);
            for (int k = 0; k < nb; ++k) {
                const double ck = (k == 0 || k == N / 2) ? 1.0 : 2.0;
                const double ang = 2.0 * M_PI * (double)((long)k * n % N) / N;
                const float cr = (float)(win * ck * cos(ang) / N);
                const float ci = (k == 0 || k == N / 2) ? 0.f : (float)(-win * ck * sin(ang) / N);
                if (c->fmt == kOpF16) {       // ONE fp16 term per bin, basis scaled by 2^9 into fp16's normal range (codec.h kDftScale; ola_kernel takes it back)
                    bf16_t* row = &B[(size_t)n * K3];
                    row[k] = h_f2h(cr * kDftScale); row[nb + k] = h_f2h(ci * kDftScale);
                    continue;
                }
                const bf16_t crh = h_f2bf(cr), cih = h_f2bf(ci);
                const bf16_t crl = h_f2bf(cr - h_bf2f(crh)), cil = h_f2bf(ci - h_bf2f(cih));
                bf16_t* row = &B[(size_t)n * K3];
                row[k] = crh; row[nb + k] = cih;
                row[2 * nb + k] = crh; row[3 * nb + k] = cih;
                row[4 * nb + k] = crl; row[5 * nb + k] = cil;
            }
        }
        if (dalloc(c, &c->basis3, B.size()) != NTTS_OK) return NTTS_ENOMEM;
        CHIP(c, hipMemcpy(c->basis3, B.data(), B.size() * 2, hipMemcpyHostToDevice));
        c->win2 = f.up_f32(w2);
    }
    if (f.rc != NTTS_OK) return f.rc;
    c->host.clear();
    c->finalized = true;
    return NTTS_OK;
}

static GemmArgs cg(const bf16_t* X, long ldx, const bf16_t* W, long K, const float* bias, void* out, long ldo, long M, int N,
                   const float* resid = nullptr, long ldr = 0) {
    GemmArgs a{};
    a.X = X; a.ldx = ldx; a.W = W; a.ldw = K; a.bias_f32 = bias; a.out = out; a.ldo = ldo; a.M = (int)M; a.N = N; a.K = (int)K;
    a.resid = resid; a.ldr = ldr;
    return a;
}

// big-M GEMM of the codec on the engine's operand format
#define CGEMM(EPI, ga, st) do { if (c->fmt == kOpF16) NTTS_GEMM_BIG_F16(EPI, ga, st); else NTTS_GEMM_BIG(EPI, ga, st); } while (0)

static void resnet_block(ntts_codec* c, const ResW& w, const CodecRows& R, long rows) {
    const int H = c->H;
    hipStream_t st = c->stream;
    GroupNormArgs g{};
    const long S = c->S;          // split operand rows: 3 x the columns, on the X side (ldx, K) and in the packed weights alike
    g.x = c->h; g.y = c->xa; g.gamma = w.g1; g.beta = w.b1; g.R = R; g.C = H; g.eps = 1e-6f; g.split = c->fmt;
    groupnorm_silu_launch(g, c->gn_reg ? R.Tp - 2 * kPadRows : (1 << 30), st);
    { GemmArgs ga_ = cg(c->xa, S * H, w.w1, 3L * S * H, w.cb1, c->t1 + H, H, rows - 2, H); CGEMM(EPI_F32, ga_, st); }
    g.x = c->t1; g.y = c->xb; g.gamma = w.g2; g.beta = w.b2;
    groupnorm_silu_launch(g, c->gn_reg ? R.Tp - 2 * kPadRows : (1 << 30), st);
    { GemmArgs ga_ = cg(c->xb, S * H, w.w2, 3L * S * H, w.cb2, c->h + H, H, rows - 2, H, c->h + H, H); CGEMM(EPI_F32, ga_, st); }
}

// ---- output stage (ntts_wav_format; kernels/codec.h wav_format_kernel).  The reference has none: its users' torchaudio.functional.resample and
// int16 cast sit behind ref:neutts/neutts.py:288-291 on the host.
struct WavFmt {
    int rate = 24000, enc = NTTS_WAV_F32, W = 6, orig = 1, nw = 1;
    size_t esz = 4;
    bool plain() const { return rate == 24000 && enc == NTTS_WAV_F32; }     // the engine's native output: no kernel, no second buffer
    int64_t out_len(int64_t n_in) const { return (n_in * nw + orig - 1) / orig; }
};
// a null format is the zeroed one: 24 000 Hz / float32 / width 6
static int wav_fmt_check(ntts_codec* c, const ntts_wav_format* f, WavFmt* o) {
    static const int rates[] = {8000, 16000, 22050, 24000, 32000, 44100, 48000};
    WavFmt w;
    if (f) {
        if (f->sample_rate) w.rate = f->sample_rate;
        w.enc = f->encoding;
        if (f->filter_width < 0 || f->filter_width > 64) return cfail(c, NTTS_EINVAL, "wav format: filter_width %d outside [0, 64] (0 = 6)", f->filter_width);
        if (f->filter_width) w.W = f->filter_width;
    }
    if (std::find(std::begin(rates), std::end(rates), w.rate) == std::end(rates))
        return cfail(c, NTTS_EINVAL, "wav format: sample_rate %d is not one of 8000, 16000, 22050, 24000, 32000, 44100, 48000", w.rate);
    if (w.enc != NTTS_WAV_F32 && w.enc != NTTS_WAV_PCM16 && w.enc != NTTS_WAV_MULAW)
        return cfail(c, NTTS_EINVAL, "wav format: unknown encoding %d (0 = float32, 1 = PCM16, 2 = mu-law)", w.enc);
    const int g = std::gcd(24000, w.rate);
    w.orig = 24000 / g; w.nw = w.rate / g;
    w.esz = w.enc == NTTS_WAV_F32 ? 4 : w.enc == NTTS_WAV_PCM16 ? 2 : 1;
    *o = w;
    return NTTS_OK;
}

extern "C" int ntts_wav_out_len(const ntts_wav_format* fmt, int64_t n_in, int64_t* n_out) {
    WavFmt w;
    if (!n_out || n_in < 0) return cfail(nullptr, NTTS_EINVAL, "ntts_wav_out_len: null / negative argument");
    const int rc = wav_fmt_check(nullptr, fmt, &w);
    if (rc != NTTS_OK) return rc;
    *n_out = w.out_len(n_in);
    return NTTS_OK;
}

// the [taps][nw] fp32 table of a (rate, width) pair: built in double, rounded once, uploaded on first use, kept until destroy
static int wav_table(ntts_codec* c, const WavFmt& w, ntts_codec::WavTable* out) {
    const auto key = std::make_pair(w.rate, w.W);
    auto it = c->wav_tables.find(key);
    if (it != c->wav_tables.end()) { *out = it->second; return NTTS_OK; }
    const int orig = w.orig, nw = w.nw;
    const double base = std::min(orig, nw) * 0.99;                    // rolloff 0.99 of the lower Nyquist frequency
    const int width = (int)ceil((double)w.W * orig / base), taps = 2 * width + orig;
    if (((kWavBlock - 1) / nw + 1) * orig + taps > kWavSpanMax) return cfail(c, NTTS_EINVAL, "wav format: filter of %d taps exceeds the kernel's staging span", taps);
    std::vector<float> h((size_t)taps * nw);
    for (int p = 0; p < nw; ++p)
        for (int j = 0; j < taps; ++j) {
            double t = (-(double)p / nw + (double)(j - width) / orig) * base;
            t = std::min(std::max(t, -(double)w.W), (double)w.W);
            const double win = cos(M_PI * t / (2.0 * w.W));
            const double snc = t == 0.0 ? 1.0 : sin(M_PI * t) / (M_PI * t);
            h[(size_t)j * nw + p] = (float)(snc * win * win * (base / orig));
        }
    ntts_codec::WavTable tb{nullptr, orig, nw, width, taps};
    const int rc = dalloc(c, &tb.coef, h.size());
    if (rc != NTTS_OK) return rc;
    CHIP(c, hipMemcpy(tb.coef, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    c->wav_tables[key] = tb;
    *out = tb;
    return NTTS_OK;
}

// Room for `need` elements in a stage's buffer.  The first call that needs it (or a larger one) allocates max(need, whole), `whole` being what the
// engine's whole waveform workspace can ask of this buffer; the stream is drained first: a kernel queued on it may still read the old one.
template <typename T>
static int grow(ntts_codec* c, ntts_codec::Grown<T>& b, size_t need, size_t whole, hipStream_t st) {
    if (b.cap >= need) return NTTS_OK;
    CHIP(c, hipStreamSynchronize(st));
    if (b.p) { hipFree(b.p); b.p = nullptr; b.cap = 0; }
    CHIP(c, hipMalloc((void**)&b.p, std::max(need, whole) * sizeof(T)));
    b.cap = std::max(need, whole);
    return NTTS_OK;
}

// in [n][in_stride] (utterance b: lens_dev[b] * len_mul samples; the rest of a row is scratch) -> c->fbuf [n][out_len_max] in the format's element type
static int wav_format_launch(ntts_codec* c, const WavFmt& w, const float* in, long in_stride, const int* lens_dev, int len_mul, int n,
                             int64_t out_len_max, hipStream_t st) {
    // (a wider format grows it: room for the engine's whole waveform workspace in this format)
    int rc = grow(c, c->fbuf, (size_t)n * out_len_max * w.esz, ((size_t)w.out_len((int64_t)c->wav_cap) + (size_t)c->max_rows) * w.esz, st);
    if (rc != NTTS_OK) return rc;
    WavFormatArgs a{};
    a.in = in; a.in_stride = in_stride; a.lens = lens_dev; a.len_mul = len_mul; a.out = c->fbuf.p; a.out_stride = out_len_max; a.enc = w.enc;
    a.orig = 1; a.nw = 1;
    if (w.rate != 24000) {
        ntts_codec::WavTable tb;
        rc = wav_table(c, w, &tb);
        if (rc != NTTS_OK) return rc;
        a.coef = tb.coef; a.orig = tb.orig; a.nw = tb.nw; a.width = tb.width; a.taps = tb.taps;
    }
    NTTS_LAUNCH((wav_format_kernel), dim3(n, (unsigned)((out_len_max + kWavBlock - 1) / kWavBlock)), dim3(256), st, a);
    return NTTS_OK;
}

// ---- time stretch between overlap-add and the output stage (kernels/codec.h wav_stretch_*; tests/time_stretch_spec.py is the contract)
static int64_t stretch_len(int64_t n_in, int pm) { return (n_in * 1000 + pm - 1) / pm; }
static int64_t stretch_frames(int64_t n_out) { return (n_out + kStretchHop - 1) / kStretchHop; }
// every speed inside [500, 2000]; *any = one of them is not 1000 (otherwise nothing of the stage is run)
static int stretch_check(ntts_codec* c, const int32_t* speed, int n, bool* any) {
    *any = false;
    for (int i = 0; i < n; ++i) {
        if (speed[i] < 500 || speed[i] > 2000) return cfail(c, NTTS_EINVAL, "utterance %d: speed %d per mille outside [500, 2000]", i, speed[i]);
        if (speed[i] != 1000) *any = true;
    }
    if (*any && (int64_t)c->cfg.max_frames * c->cfg.hop_length >= (1 << 22))
        return cfail(c, NTTS_EINVAL, "speed: an engine of %ld samples per utterance exceeds the search kernel's 2^22", (long)c->cfg.max_frames * c->cfg.hop_length);
    return NTTS_OK;
}

extern "C" int ntts_wav_stretch_len(int32_t speed_permille, int64_t n_in, int64_t* n_out) {
    if (!n_out || n_in < 0) return cfail(nullptr, NTTS_EINVAL, "ntts_wav_stretch_len: null / negative argument");
    if (speed_permille < 500 || speed_permille > 2000) return cfail(nullptr, NTTS_EINVAL, "ntts_wav_stretch_len: speed %d per mille outside [500, 2000]", speed_permille);
    *n_out = stretch_len(n_in, speed_permille);
    return NTTS_OK;
}

// in [n][in_stride] (utterance b: lens_dev[b] * len_mul samples, speed pm_dev[b], nout_dev[b] output samples) -> c->sbuf [n][n_out_max] float32,
// c->spos [n][stretch_frames(n_out_max)]
static int wav_stretch_launch(ntts_codec* c, const float* in, long in_stride, const int* lens_dev, int len_mul, const int* pm_dev, const int* nout_dev,
                              int n, int64_t n_out_max, hipStream_t st) {
    const int64_t k_max = stretch_frames(n_out_max);
    if (!c->sfade) {                       // the stage's first launch on this engine: the fade table and the events
        CHIP(c, hipStreamSynchronize(st));
        std::vector<float> f(kStretchHop);
        for (int i = 0; i < kStretchHop; ++i) f[i] = (float)(0.5 - 0.5 * cos(M_PI * (i + 0.5) / kStretchHop));
        const int rc = dalloc(c, &c->sfade, f.size());
        if (rc != NTTS_OK) return rc;
        CHIP(c, hipMemcpy(c->sfade, f.data(), f.size() * sizeof(float), hipMemcpyHostToDevice));
        for (auto& e : c->ev_s) CHIP(c, hipEventCreate(&e));
    }
    int rc = grow(c, c->sbuf, (size_t)n * n_out_max, 2 * c->wav_cap + (size_t)c->max_rows, st);
    if (rc == NTTS_OK) rc = grow(c, c->spos, (size_t)n * k_max, 2 * c->wav_cap / kStretchHop + 2 * (size_t)c->max_rows, st);
    if (rc != NTTS_OK) return rc;
    WavStretchArgs a{};
    a.in = in; a.in_stride = in_stride; a.lens = lens_dev; a.len_mul = len_mul; a.pm = pm_dev; a.n_out = nout_dev;
    a.pos = c->spos.p; a.pos_stride = k_max; a.fade = c->sfade; a.out = c->sbuf.p; a.out_stride = n_out_max;
    CHIP(c, hipEventRecord(c->ev_s[0], st));
    NTTS_LAUNCH((wav_stretch_search_kernel), dim3(n), dim3(256), st, a);
    CHIP(c, hipEventRecord(c->ev_s[1], st));
    NTTS_LAUNCH((wav_stretch_render_kernel), dim3(n, (unsigned)((n_out_max + 255) / 256)), dim3(256), st, a);
    CHIP(c, hipEventRecord(c->ev_s[2], st));
    c->have_stretch_time = true;
    return NTTS_OK;
}

// ---- loudness normalisation between the time stretch and the output stage (kernels/codec.h wav_loud_*; tests/loudness_spec.py is the contract)
// one biquad of the K-weighting at the native rate: the bilinear construction that gives the standard's 48 kHz table at 48 kHz
static void loud_biquad(double f0, double Q, double Vh, double Vb, bool shelf, double* b, double* a) {
    const double K = tan(M_PI * f0 / 24000.0), a0 = 1.0 + K / Q + K * K;
    if (shelf) { b[0] = (Vh + Vb * K / Q + K * K) / a0; b[1] = 2.0 * (K * K - Vh) / a0; b[2] = (Vh - Vb * K / Q + K * K) / a0; }
    a[0] = 2.0 * (K * K - 1.0) / a0; a[1] = (1.0 - K / Q + K * K) / a0;
}
// the parameters of every row with the option on inside their ranges (a NaN is outside); *any = one row has it on
static int loud_check(ntts_codec* c, const ntts_wav_loudness* loud, int n, bool* any) {
    *any = false;
    for (int i = 0; i < n; ++i) {
        if (!loud[i].enable) continue;
        *any = true;
        if (!(loud[i].target_lufs >= -70.f && loud[i].target_lufs <= 0.f))
            return cfail(c, NTTS_EINVAL, "utterance %d: loudness target_lufs %g outside [-70, 0]", i, (double)loud[i].target_lufs);
        if (!(loud[i].peak_dbfs >= -20.f && loud[i].peak_dbfs <= 0.f))
            return cfail(c, NTTS_EINVAL, "utterance %d: loudness peak_dbfs %g outside [-20, 0]", i, (double)loud[i].peak_dbfs);
        if (!(loud[i].max_gain_db >= 0.f && loud[i].max_gain_db <= 60.f))
            return cfail(c, NTTS_EINVAL, "utterance %d: loudness max_gain_db %g outside [0, 60]", i, (double)loud[i].max_gain_db);
    }
    return NTTS_OK;
}
// [enable, target_lufs, peak_dbfs, max_gain_db] of n rows as floats, the layout the gate kernel reads (through the int meta block)
static void loud_pack(int* dst, const ntts_wav_loudness* loud, int n) {
    for (int i = 0; i < n; ++i) {
        const float v[4] = {loud[i].enable ? 1.f : 0.f, loud[i].target_lufs, loud[i].peak_dbfs, loud[i].max_gain_db};
        memcpy(dst + 4 * (size_t)i, v, sizeof v);
    }
}

// io [n][stride] (utterance b: lens_dev[b] * len_mul samples, the longest n_max): measure every row, gate, and -- with par_dev, [n][4] floats as
// loud_pack wrote them -- scale the rows in place; without it nothing is changed.  c->lres [n][3] receives (L, peak, g).
static int wav_loud_launch(ntts_codec* c, float* io, long stride, const int* lens_dev, int len_mul, const int* par_dev, int n, int64_t n_max,
                           hipStream_t st) {
    const int64_t j_max = n_max / kLoudSub;
    const int64_t z_stride = std::max<int64_t>(j_max, 1), gy = std::max<int64_t>((j_max + kLoudLanes - 1) / kLoudLanes, 1);
    if (!c->ev_l[0]) {                     // the stage's first launch on this engine: the K-weighting coefficients and the events
        double b[3];
        loud_biquad(1681.974450955533, 0.7071752369554196, pow(10.0, 3.999843853973347 / 20.0),
                    pow(pow(10.0, 3.999843853973347 / 20.0), 0.4996667741545416), true, b, c->kw + 3);
        c->kw[0] = b[0]; c->kw[1] = b[1]; c->kw[2] = b[2];
        loud_biquad(38.13547087602444, 0.5003270373238773, 0.0, 0.0, false, nullptr, c->kw + 5);
        for (auto& e : c->ev_l) CHIP(c, hipEventCreate(&e));
    }
    // room for the whole waveform workspace: as many sub-blocks (and partial peaks of kLoudLanes of them) as it holds, one per row at least
    int rc = grow(c, c->lz, (size_t)n * z_stride, 2 * c->wav_cap / kLoudSub + (size_t)c->max_rows, st);
    if (rc == NTTS_OK) rc = grow(c, c->lpk, (size_t)n * gy, 2 * c->wav_cap / ((size_t)kLoudSub * kLoudLanes) + (size_t)c->max_rows, st);
    if (rc == NTTS_OK) rc = grow(c, c->lres, 3 * (size_t)n, 3 * (size_t)c->max_rows, st);
    if (rc != NTTS_OK) return rc;
    WavLoudArgs a{};
    a.io = io; a.stride = stride; a.lens = lens_dev; a.len_mul = len_mul; a.par = (const float*)par_dev;
    memcpy(a.kw, c->kw, sizeof a.kw);
    a.z = c->lz.p; a.z_stride = (long)z_stride; a.pk = c->lpk.p; a.pk_stride = (int)gy; a.res = c->lres.p;
    CHIP(c, hipEventRecord(c->ev_l[0], st));
    NTTS_LAUNCH((wav_loud_measure_kernel), dim3(n, (unsigned)gy), dim3(kLoudLanes), st, a);
    CHIP(c, hipEventRecord(c->ev_l[1], st));
    NTTS_LAUNCH((wav_loud_gate_kernel), dim3(n), dim3(kLoudLanes), st, a);
    CHIP(c, hipEventRecord(c->ev_l[2], st));
    if (par_dev && n_max > 0) NTTS_LAUNCH((wav_loud_apply_kernel), dim3(n, (unsigned)((n_max + 1023) / 1024)), dim3(256), st, a);
    CHIP(c, hipEventRecord(c->ev_l[3], st));
    c->have_loud_time = true;
    return NTTS_OK;
}

// ---- the stages of one call behind overlap-add, in the order they run: time stretch, loudness, output format (DESIGN.md "Output path").
// A stage that has nothing to do is off, and a call with every stage off launches nothing behind the waveform.
struct WavPost {
    WavFmt w;                                  // the checked format; its kernel runs unless it is the native one
    const int32_t* speed = nullptr;            // per mille per row; null: every row at 1000
    const ntts_wav_loudness* loud = nullptr;   // per row; null: no row has the option on
    bool measure = false;                      // the loudness kernels without a parameter block: the figures alone, nothing scaled
    bool loud_on() const { return loud || measure; }
    bool idle() const { return !speed && !loud_on() && w.plain(); }
    WavPost from_row(int i0) const {           // the same stages for the rows i0.. of the call
        WavPost q = *this;
        if (speed) q.speed += i0;
        if (loud) q.loud += i0;
        return q;
    }
};
// The caller's (fmt, speed_permille, loudness) of n rows in two steps, because a decode call's own argument checks stand between the format's check
// and the stages': wav_post_format starts the description from the checked format, wav_post_stages checks speeds and loudness and switches each
// on only where something is asked of it.  The only place where a stage is switched off.
static int wav_post_format(ntts_codec* c, const ntts_wav_format* fmt, WavPost* p) {
    *p = WavPost{};
    return wav_fmt_check(c, fmt, &p->w);
}
static int wav_post_stages(ntts_codec* c, const int32_t* speed, const ntts_wav_loudness* loud, int n, WavPost* p) {
    int rc = NTTS_OK;
    bool any = false;
    if (speed) rc = stretch_check(c, speed, n, &any);
    if (rc == NTTS_OK && any) p->speed = speed;
    any = false;
    if (rc == NTTS_OK && loud) rc = loud_check(c, loud, n, &any);
    if (rc == NTTS_OK && any) p->loud = loud;
    return rc;
}

// The meta tail of n rows of lens[i] * mul samples: [speed n][stretched samples n] with a speed, then [enable, target, peak, max gain] x n as floats
// with a loudness.  Returns its ints and, where asked, writes it (tail), every row's samples in the output format (out_lens) and the longest row
// behind the stretch at 24 kHz (s_max).
static size_t wav_post_tail(const WavPost& p, int n, const int32_t* lens, int mul, int* tail, int32_t* out_lens, int64_t* s_max) {
    int64_t longest = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t s = p.speed ? stretch_len((int64_t)mul * lens[i], p.speed[i]) : (int64_t)mul * lens[i];
        longest = std::max(longest, s);
        if (out_lens) out_lens[i] = (int32_t)p.w.out_len(s);
        if (tail && p.speed) { tail[i] = p.speed[i]; tail[n + i] = (int)s; }
    }
    if (s_max) *s_max = longest;
    const size_t ld_off = p.speed ? 2 * (size_t)n : 0;
    if (tail && p.loud) loud_pack(tail + ld_off, p.loud, n);
    return ld_off + (p.loud ? 4 * (size_t)n : 0);
}

// what a call hands over: [n][stride] elements of esz bytes at src
struct WavOut { const void* src; long stride; size_t esz; };
// The chain on n rows on the device -- in [n][stride], row b of lens_dev[b] * len_mul samples, s_max the longest behind the stretch -- with the
// call's meta tail at tail_dev (wav_post_tail).  A stretch moves the rows to c->sbuf, the loudness scales them where they stand (`in` and c->sbuf
// are this call's own), a format moves them to c->fbuf.
static int wav_post_launch(ntts_codec* c, const WavPost& p, float* in, long stride, const int* lens_dev, int len_mul, int n, int64_t s_max,
                           const int* tail_dev, hipStream_t st, WavOut* o) {
    if (p.speed) {
        const int rc = wav_stretch_launch(c, in, stride, lens_dev, len_mul, tail_dev, tail_dev + n, n, s_max, st);
        if (rc != NTTS_OK) return rc;
        in = c->sbuf.p; stride = (long)s_max; lens_dev = tail_dev + n; len_mul = 1;
        tail_dev += 2 * (size_t)n;
    }
    if (p.loud_on()) {
        const int rc = wav_loud_launch(c, in, stride, lens_dev, len_mul, p.loud ? tail_dev : nullptr, n, s_max, st);
        if (rc != NTTS_OK) return rc;
    }
    *o = WavOut{in, stride, sizeof(float)};
    if (!p.w.plain()) {
        const int64_t row_len = p.w.out_len(s_max);
        const int rc = wav_format_launch(c, p.w, in, stride, lens_dev, len_mul, n, row_len, st);
        if (rc != NTTS_OK) return rc;
        *o = WavOut{c->fbuf.p, (long)row_len, p.w.esz};
    }
    return NTTS_OK;
}

// One meta block through the page-locked ring: pack(slot) fills the next slot and returns its ints, the copy to c->meta is asynchronous (the slot is
// free again once the copy out of it, two blocks ago, has completed: no stream-wide wait)
template <typename Pack>
static int meta_send(ntts_codec* c, hipStream_t st, Pack pack) {
    const int k = c->meta_next;
    c->meta_next = (k + 1) % ntts_codec::kMetaStages;
    if (c->meta_used[k]) CHIP(c, hipEventSynchronize(c->meta_ev[k]));
    const size_t n_ints = pack(c->meta_host[k]);
    CHIP(c, hipMemcpyAsync(c->meta, c->meta_host[k], n_ints * sizeof(int), hipMemcpyHostToDevice, st));
    c->meta_used[k] = true;
    CHIP(c, hipEventRecord(c->meta_ev[k], st));
    return NTTS_OK;
}

// codes: HOST packed codes (codes_dev == null), or DEVICE codes, utterance i at codes_dev + i * codes_stride (already in range:
// they come from ntts_backbone_export_codes).  out_kind: 0 = host destination, blocking (the classic entry point);
// 1 = host destination (pinned), asynchronous; 2 = device destination, asynchronous.  producer: a HIP stream whose work so far
// must complete before the codes are read (the backbone's stream), or null.  post: the stages behind overlap-add (with none of them on the
// waveform buffer is the copy's source and nothing more is launched); wav_stride counts elements of its format, out_lens (may be null)
// receives every utterance's samples.  The arguments are codec_decode's: checked there.
static int codec_decode_impl(ntts_codec* c, int32_t n, const int32_t* codes, const int32_t* codes_dev, int32_t codes_stride,
                             const int32_t* lens, void* wav_out, int64_t wav_stride, int out_kind, hipStream_t producer,
                             const WavPost& post, int32_t* out_lens) {
    CHIP(c, hipSetDevice(c->device));
    const int H = c->H, hop = c->cfg.hop_length;
    int Tmax = 0;
    long total = 0;
    long ncodes = 1;
    for (int i = 0; i < c->nq; ++i) ncodes *= c->cfg.levels[i];
    for (int i = 0; i < n; ++i) {
        if (lens[i] < 1 || lens[i] > c->cfg.max_frames) return cfail(c, NTTS_EINVAL, "utterance %d: %d frames (1..%d)", i, lens[i], c->cfg.max_frames);
        if (lens[i] > Tmax) Tmax = lens[i];
        total += lens[i];
    }
    if (codes)
        for (long i = 0; i < total; ++i)
            if (codes[i] < 0 || codes[i] >= ncodes) return cfail(c, NTTS_EINVAL, "code %d out of range [0, %ld)", codes[i], ncodes);
    if (codes_dev && codes_stride < Tmax) return cfail(c, NTTS_EINVAL, "codes_stride %d < longest utterance %d", codes_stride, Tmax);
    // samples per row of the hand-over (the longest utterance's, in the output format) and bytes per sample
    // (with a speed: of the longest STRETCHED utterance)
    int64_t s_max;
    const size_t tail_ints = wav_post_tail(post, n, lens, hop, nullptr, nullptr, &s_max);
    const int64_t row_len = post.w.out_len(s_max);
    if (wav_stride < row_len) return cfail(c, NTTS_EINVAL, "wav_stride %ld < %ld samples", (long)wav_stride, (long)row_len);
    if (out_lens) wav_post_tail(post, n, lens, hop, nullptr, out_lens, nullptr);
    const int Tp = Tmax + 2 * kPadRows;
    const long rows = total + 2L * kPadRows * n;          // packed: every utterance brings its own frames + pad rows (codec.h)
    if (rows > c->max_rows) return cfail(c, NTTS_EINVAL, "%ld rows exceed max_rows %ld: decode fewer utterances per call", rows, c->max_rows);
    const int npages = (Tmax + kPage - 1) / kPage, qtiles = (Tmax + 63) / 64;
    // the waveform staging buffer holds n rows of the LONGEST utterance's samples (workspace rows x hop samples in all)
    if ((long)n * Tmax > c->max_rows) return cfail(c, NTTS_EINVAL, "%d utterances x %d frames exceed max_rows %ld: decode fewer utterances per call", n, Tmax, c->max_rows);
    // the V^T pages of the paged attention path are laid out per utterance x the LONGEST utterance's pages (not packed)
    if (!(c->attn_resident && npages <= kAttnResPages) && (long)n * npages * kPage > c->max_rows + (c->max_rows / (1 + 2 * kPadRows) + 1) * kPage)
        return cfail(c, NTTS_EINVAL, "%d utterances x %d pages exceed the V^T workspace: decode fewer utterances per call", n, npages);
    // ---- meta: [lens n][code_off n][row_off n + 1][codes total], built in a page-locked ring slot: the copy is asynchronous, no stream-wide wait
    // and the stages' tail (wav_post_tail) behind them
    const size_t tail_off = 3 * (size_t)n + 1 + (codes ? (size_t)total : 0);
    if (tail_off + tail_ints > c->meta_cap) return cfail(c, NTTS_EINVAL, "meta block too large");
    hipStream_t st = c->stream;
    {
        const int rc = meta_send(c, st, [&](int* m) {
            size_t at = 0;
            memcpy(m, lens, (size_t)n * sizeof(int)); at = n;
            long off = 0;
            for (int i = 0; i < n; ++i) { m[at++] = codes ? (int)off : i * codes_stride; off += lens[i]; }
            long roff = 0;
            for (int i = 0; i < n; ++i) { m[at++] = (int)roff; roff += lens[i] + 2 * kPadRows; }
            m[at++] = (int)roff;
            if (codes) { memcpy(m + at, codes, (size_t)total * sizeof(int)); at += total; }
            return at + wav_post_tail(post, n, lens, hop, m + at, nullptr, nullptr);
        });
        if (rc != NTTS_OK) return rc;
    }
    if (producer) {                        // the codes are being written on another stream: order this pass behind it
        CHIP(c, hipEventRecord(c->ev_in, producer));
        CHIP(c, hipStreamWaitEvent(st, c->ev_in, 0));
    }
    CodecRows R{c->meta, c->meta + 2 * n, n, Tp, rows};
    CHIP(c, hipEventRecord(c->ev[0], st));

    CodecEmbedArgs ea{};
    const long S = c->S;
    ea.codes = codes ? c->meta + 3 * n + 1 : codes_dev; ea.code_off = c->meta + n; ea.wf = c->wf; ea.bf = c->bf; ea.out = c->xa; ea.R = R; ea.H = H; ea.nq = c->nq; ea.split = c->fmt;
    for (int i = 0; i < 8; ++i) ea.levels[i] = i < c->nq ? c->cfg.levels[i] : 1;
    NTTS_LAUNCH((codec_embed_kernel), dim3((unsigned)((rows + kEmbedRows - 1) / kEmbedRows)), dim3(256), st, ea);
    // stem Conv1d(k=7, padding 3): window rows r..r+6 -> centre row r+3
    { GemmArgs ga_ = cg(c->xa, S * H, c->embed_w, 7L * S * H, c->embed_b, c->h + 3L * H, H, rows - 6, H); CGEMM(EPI_F32, ga_, st); }
    auto tap = [&](int stage) -> hipError_t {   // debug only: the residual stream after a stage (hf:models/xcodec2/modeling_xcodec2.py:841-859)
        if (!c->tap) return hipSuccess;
        return hipMemcpyAsync(c->tap + (size_t)stage * c->max_rows * H, c->h, (size_t)rows * H * sizeof(float), hipMemcpyDeviceToDevice, st);
    };
    if (c->tap) {
        c->tap_off.assign(n, 0); c->tap_len.assign(lens, lens + n);
        long ro = 0;
        for (int i = 0; i < n; ++i) { c->tap_off[i] = (int)ro; ro += lens[i] + 2 * kPadRows; }
    }
    CHIP(c, tap(0));
    resnet_block(c, c->res[0], R, rows);
    resnet_block(c, c->res[1], R, rows);
    CHIP(c, tap(1));
    for (int i = 0; i < c->cfg.num_layers; ++i) {
        const CLayerW& L = c->layers[i];
        RowNormArgs rn{};
        rn.x = c->h; rn.y = c->xa; rn.w = L.ln1; rn.rows = rows; rn.C = H; rn.eps = c->cfg.rms_eps; rn.split = c->fmt;
        rownorm_launch(rn, st);
        { GemmArgs ga_ = cg(c->xa, S * H, L.wqkv, S * H, nullptr, c->qkv, 3L * H, rows, 3 * H); CGEMM(EPI_BF16, ga_, st); }
        AttnFullArgs at{};
        at.qkv = c->qkv; at.vt = c->vt; at.out = c->xb; at.R = R; at.C = H; at.nh = c->cfg.num_heads; at.npages = npages; at.qtiles = qtiles; at.split = c->fmt;
        if (c->attn_resident && npages <= kAttnResPages) {   // up to 256 frames: K / V^T resident in LDS, one sweep, no V^T pass
            const dim3 ag(n, c->cfg.num_heads);
            if (c->fmt == kOpF16) {
                if (npages <= 8) NTTS_LAUNCH((attn_full_resident_kernel<8, true>), ag, dim3(512), st, at);
                else if (npages <= 12) NTTS_LAUNCH((attn_full_resident_kernel<12, true>), ag, dim3(512), st, at);
                else NTTS_LAUNCH((attn_full_resident_kernel<16, true>), ag, dim3(512), st, at);
            } else {
                if (npages <= 8) NTTS_LAUNCH((attn_full_resident_kernel<8, false>), ag, dim3(512), st, at);
                else if (npages <= 12) NTTS_LAUNCH((attn_full_resident_kernel<12, false>), ag, dim3(512), st, at);
                else NTTS_LAUNCH((attn_full_resident_kernel<16, false>), ag, dim3(512), st, at);
            }
        } else {
            VTransposeArgs vt{};
            vt.qkv = c->qkv; vt.vt = c->vt; vt.R = R; vt.C = H; vt.nh = c->cfg.num_heads; vt.npages = npages;
            NTTS_LAUNCH((v_transpose_kernel), dim3(n * npages, c->cfg.num_heads), dim3(256), st, vt);
            if (c->fmt == kOpF16) NTTS_LAUNCH((attn_full_kernel<true>), dim3(n * qtiles, c->cfg.num_heads), dim3(256), st, at);
            else NTTS_LAUNCH((attn_full_kernel<false>), dim3(n * qtiles, c->cfg.num_heads), dim3(256), st, at);
        }
        { GemmArgs ga_ = cg(c->xb, S * H, L.wo, S * H, nullptr, c->h, H, rows, H, c->h, H); CGEMM(EPI_F32, ga_, st); }
        rn.w = L.ln2;
        rownorm_launch(rn, st);
        { GemmArgs ga_ = cg(c->xa, S * H, L.fc1, S * H, nullptr, c->act, S * c->I, rows, c->I);
          if (S > 1) NTTS_GEMM_BIG(EPI_SILU_SPLIT3, ga_, st); else CGEMM(EPI_BF16_SILU, ga_, st); }
        { GemmArgs ga_ = cg(c->act, S * c->I, L.fc2, S * c->I, nullptr, c->h, H, rows, H, c->h, H); CGEMM(EPI_F32, ga_, st); }
    }
    CHIP(c, tap(2));
    resnet_block(c, c->res[2], R, rows);
    resnet_block(c, c->res[3], R, rows);
    CHIP(c, tap(3));
    RowNormArgs fn{};
    fn.x = c->h; fn.y = c->xa; fn.w = c->fn_w; fn.bias = c->fn_b; fn.rows = rows; fn.C = H; fn.eps = 1e-6f; fn.split = c->fmt;
    rownorm_launch(fn, st);
    { GemmArgs ga_ = cg(c->xa, S * H, c->head_w, S * H, c->head_b, c->spec, c->lds_spec, rows, c->NS); CGEMM(EPI_F32, ga_, st); }
    IstftPrepArgs ip{};
    ip.spec = c->spec; ip.lds = c->lds_spec; ip.s3 = c->s3; ip.K3 = c->K3; ip.rows = rows; ip.nb = c->nb; ip.f16 = c->fmt == kOpF16;
    NTTS_LAUNCH((istft_prep_kernel), dim3((unsigned)rows), dim3(256), st, ip);
    { GemmArgs ga_ = cg(c->s3, c->K3, c->basis3, c->K3, nullptr, c->frames, c->n_fft, rows, c->n_fft); CGEMM(EPI_F32, ga_, st); }
    OlaArgs oa{};
    oa.frames = c->frames; oa.win2 = c->win2; oa.wav = c->wav; oa.wav_stride = (long)hop * Tmax; oa.R = R; oa.hop = hop; oa.n_fft = c->n_fft;
    oa.scale = c->fmt == kOpF16 ? 1.0f / kDftScale : 1.0f;
    NTTS_LAUNCH((ola_kernel), dim3(n, (unsigned)(((long)hop * Tmax + 255) / 256)), dim3(256), st, oa);
    WavOut o;
    {
        const int rc = wav_post_launch(c, post, c->wav, (long)hop * Tmax, R.lens, hop, n, s_max, c->meta + tail_off, st, &o);
        if (rc != NTTS_OK) return rc;
    }
    CHIP(c, hipEventRecord(c->ev[1], st));
    c->have_time = true;
    const hipMemcpyKind kind = out_kind == 2 ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    const void* src = o.src;
    const size_t esz = o.esz, row_bytes = (size_t)row_len * esz, src_pitch = (size_t)o.stride * esz;
    const bool dense = wav_stride == row_len && o.stride == row_len;      // source and destination rows back to back: one linear copy
    if (out_kind == 0) {
        CHIP(c, hipStreamSynchronize(st));
        CHIP(c, hipGetLastError());
        // one strided device-to-host copy for the whole batch (rows shorter than Tmax carry don't-care tails)
        if (dense)                   // (DMA engine at PCIe speed into pinned memory)
            CHIP(c, hipMemcpy(wav_out, src, (size_t)n * row_bytes, kind));
        else
            CHIP(c, hipMemcpy2D(wav_out, (size_t)wav_stride * esz, src, src_pitch, row_bytes, n, kind));
        return NTTS_OK;
    }
    // asynchronous hand-over, stream-ordered behind the pass (ntts_codec_sync waits for it)
    if (dense)
        CHIP(c, hipMemcpyAsync(wav_out, src, (size_t)n * row_bytes, kind, st));
    else
        CHIP(c, hipMemcpy2DAsync(wav_out, (size_t)wav_stride * esz, src, src_pitch, row_bytes, n, kind, st));
    if (c->ev_done && hipEventRecord(c->ev_done, st) == hipSuccess) c->have_done = true;
    else { (void)hipGetLastError(); c->have_done = false; }
    return NTTS_OK;
}

// Every decode entry point.  codes: on the host (out_kind 0) or on the device.  classic: ntts_codec_decode / _dev, which hand out no lengths and
// report a null engine through the global error string; the others return NTTS_EINVAL for it.  A null format, speed or loudness is that stage off.
static int codec_decode(ntts_codec* c, bool classic, int32_t n, const int32_t* codes, int32_t codes_stride, const int32_t* lens,
                        const int32_t* speed_permille, const ntts_wav_loudness* loudness, const ntts_wav_format* fmt, void* out, int64_t out_stride,
                        int out_kind, void* producer_stream, int32_t* out_lens) {
    if (!c && !classic) return NTTS_EINVAL;
    if (!codes || (!out_lens && !classic)) return cfail(c, NTTS_EINVAL, "null/empty argument");
    WavPost post;
    int rc = wav_post_format(c, fmt, &post);
    if (rc != NTTS_OK) return rc;
    if (!c || n < 1 || !lens || !out) return cfail(c, NTTS_EINVAL, "null/empty argument");
    if (!c->finalized) return cfail(c, NTTS_ESTATE, "weights not finalised");
    rc = wav_post_stages(c, speed_permille, loudness, n, &post);
    if (rc != NTTS_OK) return rc;
    return codec_decode_impl(c, n, out_kind ? nullptr : codes, out_kind ? codes : nullptr, codes_stride, lens, out, out_stride, out_kind,
                             (hipStream_t)producer_stream, post, out_lens);
}

extern "C" int ntts_codec_decode(ntts_codec* c, int32_t n, const int32_t* codes, const int32_t* lens, float* wav_out,
                                 int64_t wav_stride) {
    return codec_decode(c, true, n, codes, 0, lens, nullptr, nullptr, nullptr, wav_out, wav_stride, 0, nullptr, nullptr);
}
extern "C" int ntts_codec_decode_dev(ntts_codec* c, int32_t n, const int32_t* codes_dev, int32_t codes_stride, const int32_t* lens,
                                     float* wav_out, int64_t wav_stride, int32_t wav_on_device, void* producer_stream) {
    return codec_decode(c, true, n, codes_dev, codes_stride, lens, nullptr, nullptr, nullptr, wav_out, wav_stride, wav_on_device ? 2 : 1, producer_stream, nullptr);
}
// The same two passes with the output stage behind overlap-add (ntts_wav_format); a zeroed or null format is the plain pass, bit for bit.
extern "C" int ntts_codec_decode_fmt(ntts_codec* c, int32_t n, const int32_t* codes, const int32_t* lens, const ntts_wav_format* fmt,
                                     void* out, int64_t out_stride, int32_t* out_lens) {
    return codec_decode(c, false, n, codes, 0, lens, nullptr, nullptr, fmt, out, out_stride, 0, nullptr, out_lens);
}
extern "C" int ntts_codec_decode_dev_fmt(ntts_codec* c, int32_t n, const int32_t* codes_dev, int32_t codes_stride, const int32_t* lens,
                                         void* out, int64_t out_stride, int32_t out_on_device, void* producer_stream,
                                         const ntts_wav_format* fmt, int32_t* out_lens) {
    return codec_decode(c, false, n, codes_dev, codes_stride, lens, nullptr, nullptr, fmt, out, out_stride, out_on_device ? 2 : 1, producer_stream, out_lens);
}
// ... with a speed per utterance (per mille; null = all 1000: the very same calls)
extern "C" int ntts_codec_decode_speed(ntts_codec* c, int32_t n, const int32_t* codes, const int32_t* lens, const int32_t* speed_permille,
                                       const ntts_wav_format* fmt, void* out, int64_t out_stride, int32_t* out_lens) {
    return codec_decode(c, false, n, codes, 0, lens, speed_permille, nullptr, fmt, out, out_stride, 0, nullptr, out_lens);
}
extern "C" int ntts_codec_decode_dev_speed(ntts_codec* c, int32_t n, const int32_t* codes_dev, int32_t codes_stride, const int32_t* lens,
                                           const int32_t* speed_permille, void* out, int64_t out_stride, int32_t out_on_device,
                                           void* producer_stream, const ntts_wav_format* fmt, int32_t* out_lens) {
    return codec_decode(c, false, n, codes_dev, codes_stride, lens, speed_permille, nullptr, fmt, out, out_stride, out_on_device ? 2 : 1, producer_stream, out_lens);
}
// ... and with a loudness per utterance (null, or every enable 0: the very same calls)
extern "C" int ntts_codec_decode_loud(ntts_codec* c, int32_t n, const int32_t* codes, const int32_t* lens, const int32_t* speed_permille,
                                      const ntts_wav_loudness* loudness, const ntts_wav_format* fmt, void* out, int64_t out_stride,
                                      int32_t* out_lens) {
    return codec_decode(c, false, n, codes, 0, lens, speed_permille, loudness, fmt, out, out_stride, 0, nullptr, out_lens);
}
extern "C" int ntts_codec_decode_dev_loud(ntts_codec* c, int32_t n, const int32_t* codes_dev, int32_t codes_stride, const int32_t* lens,
                                          const int32_t* speed_permille, const ntts_wav_loudness* loudness, void* out, int64_t out_stride,
                                          int32_t out_on_device, void* producer_stream, const ntts_wav_format* fmt, int32_t* out_lens) {
    return codec_decode(c, false, n, codes_dev, codes_stride, lens, speed_permille, loudness, fmt, out, out_stride, out_on_device ? 2 : 1, producer_stream, out_lens);
}

// The chain alone on the caller's 24 kHz float32 waveforms -- HOST [n][in_stride], row i of n_samples[i] -- in rounds of as many rows as the
// waveform workspace and the meta block hold: H2D, the stages, D2H.  Blocking.  out [n][out_stride] elements of the format and out_lens (both null:
// nothing is handed out), positions [n][pos_stride] (may be null; row i receives its own K_i, nothing behind them), measured [n][3] doubles (may be
// null; needs the loudness kernels on).
static int wav_rounds(ntts_codec* c, int32_t n, const float* wav, int64_t in_stride, const int32_t* n_samples, const WavPost& post, void* out,
                      int64_t out_stride, int32_t* out_lens, int32_t* positions, int64_t pos_stride, double* measured) {
    const int64_t cap = (int64_t)c->cfg.max_frames * c->cfg.hop_length;
    int64_t Lmax = 0, s_max;
    for (int i = 0; i < n; ++i) {
        if (n_samples[i] < 0 || n_samples[i] > in_stride)
            return cfail(c, NTTS_EINVAL, "utterance %d: n_samples %d outside [0, in_stride %ld]", i, n_samples[i], (long)in_stride);
        if (n_samples[i] > cap) return cfail(c, NTTS_EINVAL, "utterance %d: %d samples exceed the engine's %ld (max_frames x hop)", i, n_samples[i], (long)cap);
        Lmax = std::max<int64_t>(Lmax, n_samples[i]);
    }
    wav_post_tail(post, n, n_samples, 1, nullptr, nullptr, &s_max);
    const int64_t row_len = post.w.out_len(s_max), k_max = stretch_frames(s_max);
    if (out && out_stride < row_len) return cfail(c, NTTS_EINVAL, "out_stride %ld < %ld samples", (long)out_stride, (long)row_len);
    if (positions && pos_stride < k_max) return cfail(c, NTTS_EINVAL, "pos_stride %ld < %ld frames", (long)pos_stride, (long)k_max);
    if (out_lens) wav_post_tail(post, n, n_samples, 1, nullptr, out_lens, nullptr);
    if (Lmax == 0) {                       // nothing but empty rows: unmeasurable, nothing to launch
        if (measured)
            for (int i = 0; i < n; ++i) { measured[3 * i] = NAN; measured[3 * i + 1] = 0.0; measured[3 * i + 2] = 1.0; }
        return NTTS_OK;
    }
    if (post.idle())                       // every stage off: nothing to compute, nothing is launched
        for (int i = 0; i < n; ++i) memcpy((float*)out + (size_t)i * out_stride, wav + (size_t)i * in_stride, (size_t)n_samples[i] * sizeof(float));
    if (positions && !post.speed)          // unit speed: frame k was taken from k * hop, by definition
        for (int i = 0; i < n; ++i)
            for (int64_t k = 0; k < stretch_frames(n_samples[i]); ++k) positions[(size_t)i * pos_stride + k] = (int32_t)(k * kStretchHop);
    if (post.idle()) return NTTS_OK;
    CHIP(c, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const int per_round = (int)std::min<int64_t>(std::min<int64_t>((int64_t)c->wav_cap / Lmax, c->max_rows),
                                                 (int64_t)c->meta_cap / (1 + (post.speed ? 2 : 0) + (post.loud_on() ? 4 : 0)));
    std::vector<int32_t> pos_host;
    for (int i0 = 0; i0 < n; i0 += per_round) {
        const int nb = std::min(per_round, n - i0);
        const WavPost rows = post.from_row(i0);
        int rc = meta_send(c, st, [&](int* m) {           // [samples nb], then the stages' tail
            memcpy(m, n_samples + i0, (size_t)nb * sizeof(int));
            return nb + wav_post_tail(rows, nb, n_samples + i0, 1, m + nb, nullptr, nullptr);
        });
        if (rc != NTTS_OK) return rc;
        CHIP(c, hipMemcpy2DAsync(c->wav, (size_t)Lmax * sizeof(float), wav + (size_t)i0 * in_stride, (size_t)in_stride * sizeof(float),
                                 (size_t)Lmax * sizeof(float), nb, hipMemcpyHostToDevice, st));
        CHIP(c, hipEventRecord(c->ev[0], st));
        WavOut o;
        rc = wav_post_launch(c, rows, c->wav, (long)Lmax, c->meta, 1, nb, s_max, c->meta + nb, st, &o);
        if (rc != NTTS_OK) return rc;
        CHIP(c, hipEventRecord(c->ev[1], st));
        c->have_time = true;
        if (out)
            CHIP(c, hipMemcpy2DAsync((char*)out + (size_t)i0 * out_stride * o.esz, (size_t)out_stride * o.esz, o.src, (size_t)o.stride * o.esz,
                                     (size_t)row_len * o.esz, nb, hipMemcpyDeviceToHost, st));
        if (positions && post.speed) {
            pos_host.resize((size_t)nb * k_max);
            CHIP(c, hipMemcpyAsync(pos_host.data(), c->spos.p, pos_host.size() * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        }
        if (measured) CHIP(c, hipMemcpyAsync(measured + 3 * (size_t)i0, c->lres.p, 3 * (size_t)nb * sizeof(double), hipMemcpyDeviceToHost, st));
        CHIP(c, hipStreamSynchronize(st));
        CHIP(c, hipGetLastError());
        if (positions && post.speed)
            for (int i = 0; i < nb; ++i)
                memcpy(positions + (size_t)(i0 + i) * pos_stride, pos_host.data() + (size_t)i * k_max,
                       (size_t)stretch_frames(stretch_len(n_samples[i0 + i], rows.speed[i])) * sizeof(int32_t));
    }
    return NTTS_OK;
}

// The output stage alone on the caller's 24 kHz float32 waveforms (a watermarker, a host library, sits between the codec and the output).
extern "C" int ntts_codec_convert(ntts_codec* c, int32_t n, const float* wav, int64_t in_stride, const int32_t* n_samples,
                                  const ntts_wav_format* fmt, void* out, int64_t out_stride, int32_t* out_lens) {
    if (!c) return NTTS_EINVAL;
    if (n < 1 || !wav || !n_samples || !out || !out_lens || in_stride < 0) return cfail(c, NTTS_EINVAL, "null/empty argument");
    WavPost post;
    const int rc = wav_post_format(c, fmt, &post);
    if (rc != NTTS_OK) return rc;
    return wav_rounds(c, n, wav, in_stride, n_samples, post, out, out_stride, out_lens, nullptr, 0, nullptr);
}

// The time stretch (and the output stage behind it) alone on the caller's 24 kHz float32 waveforms: ntts_codec_convert's twin.  Blocking.
extern "C" int ntts_codec_stretch(ntts_codec* c, int32_t n, const float* wav, int64_t in_stride, const int32_t* n_samples,
                                  const int32_t* speed_permille, const ntts_wav_format* fmt, void* out, int64_t out_stride, int32_t* out_lens,
                                  int32_t* positions, int64_t pos_stride) {
    if (!c) return NTTS_EINVAL;
    if (n < 1 || !wav || !n_samples || !speed_permille || !out || !out_lens || in_stride < 0) return cfail(c, NTTS_EINVAL, "null/empty argument");
    WavPost post;
    int rc = wav_post_format(c, fmt, &post);
    if (rc == NTTS_OK) rc = wav_post_stages(c, speed_permille, nullptr, n, &post);
    if (rc != NTTS_OK) return rc;
    return wav_rounds(c, n, wav, in_stride, n_samples, post, out, out_stride, out_lens, positions, pos_stride, nullptr);
}

// GPU milliseconds of the two kernels of the most recent time stretch (search, render)
extern "C" int ntts_codec_last_stretch_timing(ntts_codec* c, float* search_ms, float* render_ms) {
    if (!c || !search_ms || !render_ms) return NTTS_EINVAL;
    if (!c->have_stretch_time) return cfail(c, NTTS_ESTATE, "no time stretch has run on this engine");
    CHIP(c, hipSetDevice(c->device));
    CHIP(c, hipEventSynchronize(c->ev_s[2]));
    CHIP(c, hipEventElapsedTime(search_ms, c->ev_s[0], c->ev_s[1]));
    CHIP(c, hipEventElapsedTime(render_ms, c->ev_s[1], c->ev_s[2]));
    return NTTS_OK;
}

// The loudness stage (and the output stage behind it) alone on the caller's 24 kHz float32 waveforms: their twin.  measured (may be null): (L, peak, g)
// per row.  Blocking.
extern "C" int ntts_codec_normalize(ntts_codec* c, int32_t n, const float* wav, int64_t in_stride, const int32_t* n_samples,
                                    const ntts_wav_loudness* loudness, const ntts_wav_format* fmt, void* out, int64_t out_stride, int32_t* out_lens,
                                    double* measured) {
    if (!c) return NTTS_EINVAL;
    if (n < 1 || !wav || !n_samples || !loudness || !out || !out_lens || in_stride < 0) return cfail(c, NTTS_EINVAL, "null/empty argument");
    WavPost post;
    int rc = wav_post_format(c, fmt, &post);
    if (rc == NTTS_OK) rc = wav_post_stages(c, nullptr, loudness, n, &post);
    if (rc != NTTS_OK) return rc;
    if (measured) post.loud = loudness;    // somebody asks for the figures: the stage runs even with no row on (every row at gain 1)
    return wav_rounds(c, n, wav, in_stride, n_samples, post, out, out_stride, out_lens, nullptr, 0, measured);
}

// The measurement alone: no parameter block, no apply kernel, no output
extern "C" int ntts_codec_measure_loudness(ntts_codec* c, int32_t n, const float* wav, int64_t in_stride, const int32_t* n_samples,
                                           double* measured) {
    if (!c) return NTTS_EINVAL;
    if (n < 1 || !wav || !n_samples || !measured || in_stride < 0) return cfail(c, NTTS_EINVAL, "null/empty argument");
    WavPost post;
    post.measure = true;
    return wav_rounds(c, n, wav, in_stride, n_samples, post, nullptr, 0, nullptr, nullptr, 0, measured);
}

// GPU milliseconds of the measure and the apply kernel of the most recent loudness stage
extern "C" int ntts_codec_last_loudness_timing(ntts_codec* c, float* measure_ms, float* apply_ms) {
    if (!c || !measure_ms || !apply_ms) return NTTS_EINVAL;
    if (!c->have_loud_time) return cfail(c, NTTS_ESTATE, "no loudness stage has run on this engine");
    CHIP(c, hipSetDevice(c->device));
    CHIP(c, hipEventSynchronize(c->ev_l[3]));
    CHIP(c, hipEventElapsedTime(measure_ms, c->ev_l[0], c->ev_l[1]));
    CHIP(c, hipEventElapsedTime(apply_ms, c->ev_l[2], c->ev_l[3]));
    return NTTS_OK;
}

// ---- the chunked output stage (wav_stream.h; kernels/codec.h wav_stream_kernel): per-stream counts and history, shared by ntts_wav_stream_* below
// and ntts_streams_pump_end_fmt (stream.cpp)
struct ntts::WavStreamCore {
    ntts_codec* c = nullptr;
    WavFmt w;
    ntts_codec::WavTable tb{nullptr, 1, 1, 0, 0};     // coef stays null at 24 kHz
    int n = 0, max_chunk = 0, max_jobs = 0;
    long out_stride = 0, hist_stride = 0;
    std::vector<int64_t> N, M;                        // per stream: input samples received / output samples emitted
    std::vector<int> n_hist, parity;
    float* hist = nullptr;                            // device [2][n][hist_stride]
    void* out = nullptr;                              // device [max_jobs][out_stride] elements
    WavStreamJob* jobs_dev = nullptr;
    WavStreamJob* jobs_host = nullptr;                // page-locked
};

// width and taps of a checked format (wav_table's arithmetic); 0 / 0 at 24 kHz
static void wav_geometry(const WavFmt& w, int* width, int* taps) {
    if (w.rate == 24000) { *width = 0; *taps = 0; return; }
    const double base = std::min(w.orig, w.nw) * 0.99;
    *width = (int)ceil((double)w.W * w.orig / base);
    *taps = 2 * *width + w.orig;
}
static int64_t wav_count(const WavFmt& w, int width, int64_t N, bool last) {
    if (w.rate == 24000) return N;
    if (last) return w.out_len(N);
    return N >= width ? ((N - width) / w.orig) * w.nw : 0;
}

int ntts::wav_stream_count_of(ntts_codec* c, const ntts_wav_format* fmt, int64_t n_in_total, bool last, int64_t* n_out_total) {
    WavFmt w;
    if (!n_out_total || n_in_total < 0) return cfail(c, NTTS_EINVAL, "ntts_wav_stream_count: null / negative argument");
    const int rc = wav_fmt_check(c, fmt, &w);
    if (rc != NTTS_OK) return rc;
    int width, taps;
    wav_geometry(w, &width, &taps);
    *n_out_total = wav_count(w, width, n_in_total, last);
    return NTTS_OK;
}

void ntts::wav_core_destroy(WavStreamCore* k) {
    if (!k) return;
    hipSetDevice(k->c->device);
    hipStreamSynchronize(k->c->stream);
    for (void* b : {(void*)k->hist, k->out, (void*)k->jobs_dev})
        if (b) hipFree(b);
    if (k->jobs_host) hipHostFree(k->jobs_host);
    delete k;
}

int ntts::wav_core_create(ntts_codec* c, const ntts_wav_format* fmt, int n_streams, int max_chunk_samples, int max_jobs, WavStreamCore** out) {
    if (!c || !out) return NTTS_EINVAL;
    WavFmt w;
    int rc = wav_fmt_check(c, fmt, &w);
    if (rc != NTTS_OK) return rc;
    if (n_streams < 1) return cfail(c, NTTS_EINVAL, "wav stream: n_streams %d < 1", n_streams);
    if (max_chunk_samples < 1) return cfail(c, NTTS_EINVAL, "wav stream: max_chunk_samples %d < 1", max_chunk_samples);
    if (max_jobs < 1) return cfail(c, NTTS_EINVAL, "wav stream: max_jobs %d < 1", max_jobs);
    WavStreamCore* k = new WavStreamCore();
    k->c = c; k->w = w; k->n = n_streams; k->max_chunk = max_chunk_samples; k->max_jobs = max_jobs;
    k->N.assign(n_streams, 0); k->M.assign(n_streams, 0); k->n_hist.assign(n_streams, 0); k->parity.assign(n_streams, 0);
    k->out_stride = max_chunk_samples;
#define KHIP(call)                                                                                        \
    do {                                                                                                  \
        hipError_t _s = (call);                                                                           \
        if (_s != hipSuccess) {                                                                           \
            rc = cfail(c, _s == 2 ? NTTS_ENOMEM : NTTS_EHIP, "%s failed: %s", #call, hipGetErrorString(_s)); \
            wav_core_destroy(k);                                                                          \
            return rc;                                                                                    \
        }                                                                                                 \
    } while (0)
    KHIP(hipSetDevice(c->device));
    if (w.rate != 24000) {
        rc = wav_table(c, w, &k->tb);
        if (rc != NTTS_OK) { wav_core_destroy(k); return rc; }
        // a chunk emits at most the outputs of its own samples plus those the history was holding back
        k->out_stride = (long)w.out_len((int64_t)max_chunk_samples + k->tb.taps) + w.nw;
        k->hist_stride = k->tb.taps;
        KHIP(hipMalloc((void**)&k->hist, 2 * (size_t)n_streams * k->hist_stride * sizeof(float)));
        KHIP(hipMemset(k->hist, 0, 2 * (size_t)n_streams * k->hist_stride * sizeof(float)));
    }
    if (!w.plain()) {
        KHIP(hipMalloc(&k->out, (size_t)max_jobs * k->out_stride * w.esz));
        KHIP(hipMemset(k->out, 0, (size_t)max_jobs * k->out_stride * w.esz));
        KHIP(hipMalloc((void**)&k->jobs_dev, (size_t)max_jobs * sizeof(WavStreamJob)));
        KHIP(hipHostMalloc((void**)&k->jobs_host, (size_t)max_jobs * sizeof(WavStreamJob), hipHostMallocDefault));
    }
#undef KHIP
    *out = k;
    return NTTS_OK;
}

bool ntts::wav_core_plain(const WavStreamCore* k) { return k->w.plain(); }
size_t ntts::wav_core_esz(const WavStreamCore* k) { return k->w.esz; }
long ntts::wav_core_out_stride(const WavStreamCore* k) { return k->out_stride; }
void* ntts::wav_core_out(const WavStreamCore* k) { return k->out; }

int64_t ntts::wav_core_peek(const WavStreamCore* k, int u, int n_new, bool last) {
    return wav_count(k->w, k->tb.width, k->N[u] + n_new, last) - k->M[u];
}

int64_t ntts::wav_core_plan(WavStreamCore* k, int job, int u, int n_new, bool last, int phase) {
    const int64_t N1 = k->N[u] + n_new, M1 = wav_count(k->w, k->tb.width, N1, last);
    if (k->jobs_host) {
        WavStreamJob& j = k->jobs_host[job];
        j.n_before = (long)k->N[u]; j.m0 = (long)k->M[u]; j.m1 = (long)M1; j.u = u; j.n_new = n_new; j.n_hist = k->n_hist[u];
        j.parity = k->parity[u]; j.last = last ? 1 : 0; j.phase = phase;
    }
    const int64_t n_out = M1 - k->M[u];
    if (last) {                          // the stream is empty again and may start a new signal
        k->N[u] = 0; k->M[u] = 0; k->n_hist[u] = 0;
    } else {
        k->N[u] = N1; k->M[u] = M1;
        if (k->tb.coef) {
            const int64_t first = (M1 / k->w.nw) * k->w.orig - k->tb.width;
            k->n_hist[u] = (int)(N1 - (first > 0 ? first : 0));         // <= taps - 1
        }
    }
    if (k->tb.coef) k->parity[u] ^= 1;
    return n_out;
}

int ntts::wav_core_run(WavStreamCore* k, int n_jobs, const float* in_dev, long in_stride, hipStream_t st) {
    ntts_codec* c = k->c;
    if (n_jobs < 1 || k->w.plain()) return NTTS_OK;
    if (n_jobs > k->max_jobs) return cfail(c, NTTS_EINVAL, "wav stream: %d jobs exceed the %d it was created for", n_jobs, k->max_jobs);
    for (int j = 0; j < n_jobs; ++j)          // (the rows are sized for the longest chunk: checked, not assumed, before anything is written)
        if (k->jobs_host[j].m1 - k->jobs_host[j].m0 > k->out_stride || k->jobs_host[j].n_new > in_stride || k->jobs_host[j].n_hist > k->hist_stride)
            return cfail(c, NTTS_EINVAL, "wav stream: job %d (%d samples in, %ld out) exceeds its rows", j, k->jobs_host[j].n_new,
                         k->jobs_host[j].m1 - k->jobs_host[j].m0);
    CHIP(c, hipMemcpyAsync(k->jobs_dev, k->jobs_host, (size_t)n_jobs * sizeof(WavStreamJob), hipMemcpyHostToDevice, st));
    WavStreamArgs a{};
    a.f.coef = k->tb.coef; a.f.orig = k->tb.orig; a.f.nw = k->tb.nw; a.f.width = k->tb.width; a.f.taps = k->tb.taps; a.f.enc = k->w.enc;
    a.f.out = k->out; a.f.out_stride = k->out_stride;
    a.jobs = k->jobs_dev; a.in = in_dev; a.in_stride = in_stride; a.hist = k->hist; a.hist_stride = k->hist_stride; a.n_streams = k->n;
    // a stream's two jobs of one round depend on each other through its history row: two launches, phase 0 first (as the cross-fade's)
    for (int phase = 0; phase < 2; ++phase) {
        int lo = -1, hi = -1;
        int64_t longest = 0;
        for (int j = 0; j < n_jobs; ++j)
            if (k->jobs_host[j].phase == phase) {
                if (lo < 0) lo = j;
                hi = j;
                longest = std::max<int64_t>(longest, k->jobs_host[j].m1 - k->jobs_host[j].m0);
            }
        if (lo < 0) continue;
        const unsigned gy = (unsigned)std::max<int64_t>(1, (longest + kWavBlock - 1) / kWavBlock);    // (a job without output still leaves its history)
        NTTS_LAUNCH((wav_stream_kernel), dim3(hi - lo + 1, gy), dim3(256), st, a, lo, phase);
    }
    return NTTS_OK;
}

// ---- ntts_wav_stream_*: the chunked stage alone on host chunks, the streaming twin of ntts_codec_convert
struct ntts_wav_stream {
    ntts_codec* c = nullptr;
    WavStreamCore* k = nullptr;
    int n = 0, max_chunk = 0;
    float* in_dev = nullptr;             // [n][max_chunk]
    std::vector<int> seen;               // per stream: the call that named it last (repeats within one call)
    int call = 0;
    std::string err;
};
static std::string g_wav_stream_err;
// a refusal of the stream objects below: the message into its slot (the object's own error string, or its kind's global one when there is no object)
static int sfail(std::string& slot, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    slot = buf;
    return code;
}
#define WHIP(slot, call)                                                                                     \
    do {                                                                                                     \
        hipError_t _s = (call);                                                                              \
        if (_s != hipSuccess) return sfail(slot, NTTS_EHIP, "%s failed: %s", #call, hipGetErrorString(_s));   \
    } while (0)
extern "C" const char* ntts_wav_stream_last_error(const ntts_wav_stream* ws) { return ws ? ws->err.c_str() : g_wav_stream_err.c_str(); }

extern "C" void ntts_wav_stream_destroy(ntts_wav_stream* ws) {
    if (!ws) return;
    if (ws->k) wav_core_destroy(ws->k);
    if (ws->in_dev) hipFree(ws->in_dev);
    delete ws;
}

extern "C" int ntts_wav_stream_create(ntts_codec* c, const ntts_wav_format* fmt, int32_t n_streams, int32_t max_chunk_samples, ntts_wav_stream** out) {
    if (!c || !out) return sfail(g_wav_stream_err, NTTS_EINVAL, "null argument");
    ntts_wav_stream* ws = new ntts_wav_stream();
    ws->c = c; ws->n = n_streams; ws->max_chunk = max_chunk_samples;
    int rc = wav_core_create(c, fmt, n_streams, max_chunk_samples, n_streams, &ws->k);
    if (rc != NTTS_OK) { rc = sfail(g_wav_stream_err, rc, "%s", c->err.c_str()); ntts_wav_stream_destroy(ws); return rc; }
    if (!wav_core_plain(ws->k) && hipMalloc((void**)&ws->in_dev, (size_t)n_streams * max_chunk_samples * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        ntts_wav_stream_destroy(ws);
        return sfail(g_wav_stream_err, NTTS_ENOMEM, "wav stream: no device memory for %d x %d samples", n_streams, max_chunk_samples);
    }
    ws->seen.assign(n_streams, 0);
    *out = ws;
    return NTTS_OK;
}

extern "C" int ntts_wav_stream_count(const ntts_wav_format* fmt, int64_t n_in_total, int32_t last, int64_t* n_out_total) {
    const int rc = wav_stream_count_of(nullptr, fmt, n_in_total, last != 0, n_out_total);
    if (rc != NTTS_OK) sfail(g_wav_stream_err, rc, "%s", g_codec_create_err.c_str());
    return rc;
}

extern "C" int ntts_wav_stream_push(ntts_wav_stream* ws, int32_t n, const int32_t* stream, const float* wav, int64_t in_stride, const int32_t* n_samples,
                                    const int32_t* last, void* out, int64_t out_stride, int32_t* out_lens) {
    if (!ws) return NTTS_EINVAL;
    std::string& err = ws->err;
    if (n < 1 || !stream || !wav || !n_samples || !last || !out || !out_lens || in_stride < 0) return sfail(err, NTTS_EINVAL, "null/empty argument");
    // ---- every refusal first: nothing is run and no stream's state moves
    ++ws->call;
    int64_t Lmax = 0, Omax = 0;
    for (int i = 0; i < n; ++i) {
        const int u = stream[i];
        if (u < 0 || u >= ws->n) return sfail(err, NTTS_EINVAL, "entry %d: stream %d outside [0, %d)", i, u, ws->n);
        if (ws->seen[u] == ws->call) return sfail(err, NTTS_EINVAL, "entry %d: stream %d is named twice in one call", i, u);
        ws->seen[u] = ws->call;
        if (n_samples[i] < 0 || n_samples[i] > in_stride)
            return sfail(err, NTTS_EINVAL, "entry %d: n_samples %d outside [0, in_stride %ld]", i, n_samples[i], (long)in_stride);
        if (n_samples[i] > ws->max_chunk) return sfail(err, NTTS_EINVAL, "entry %d: n_samples %d above max_chunk_samples %d", i, n_samples[i], ws->max_chunk);
        Lmax = std::max<int64_t>(Lmax, n_samples[i]);
        Omax = std::max<int64_t>(Omax, wav_core_peek(ws->k, u, n_samples[i], last[i] != 0));
    }
    if (out_stride < Omax) return sfail(err, NTTS_EINVAL, "out_stride %ld < %ld samples", (long)out_stride, (long)Omax);
    for (int i = 0; i < n; ++i) out_lens[i] = (int32_t)wav_core_plan(ws->k, i, stream[i], n_samples[i], last[i] != 0, 0);
    if (wav_core_plain(ws->k)) {           // the native format: nothing to compute, nothing is launched
        for (int i = 0; i < n; ++i) memcpy((float*)out + (size_t)i * out_stride, wav + (size_t)i * in_stride, (size_t)n_samples[i] * sizeof(float));
        return NTTS_OK;
    }
    ntts_codec* c = ws->c;
    const size_t esz = wav_core_esz(ws->k);
    WHIP(err, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (Lmax > 0)
        WHIP(err, hipMemcpy2DAsync(ws->in_dev, (size_t)ws->max_chunk * sizeof(float), wav, (size_t)in_stride * sizeof(float), (size_t)Lmax * sizeof(float), n,
                              hipMemcpyHostToDevice, st));
    const int rc = wav_core_run(ws->k, n, ws->in_dev, ws->max_chunk, st);      // (also with no output at all: the histories move on)
    if (rc != NTTS_OK) return sfail(err, rc, "%s", c->err.c_str());
    if (Omax > 0)
        WHIP(err, hipMemcpy2DAsync(out, (size_t)out_stride * esz, wav_core_out(ws->k), (size_t)wav_core_out_stride(ws->k) * esz, (size_t)Omax * esz, n,
                              hipMemcpyDeviceToHost, st));
    WHIP(err, hipStreamSynchronize(st));
    WHIP(err, hipGetLastError());
    return NTTS_OK;
}

// ---- the chunked time stretch (wav_stream.h; kernels/codec.h wav_stretch_stream_kernel; tests/stream_speed_spec.py is the contract): per-stream
// counts on the host, history rows and state records on the device, shared by ntts_speed_stream_* below and ntts_streams_set_speed (stream.cpp)
struct ntts::SpeedStreamCore {
    ntts_codec* c = nullptr;
    int n = 0, max_chunk = 0, max_jobs = 0;
    long out_stride = 0, pos_stride = 0;
    std::vector<int64_t> N;                           // per stream: input samples of its current signal
    std::vector<int> pm, parity;                      // its speed (0 between signals); the history row its next job reads
    float* hist = nullptr;                            // device [2][n][kSpeedHist]
    SpeedStreamState* state = nullptr;                // device [n]
    float* fade = nullptr;                            // device [kStretchHop]
    float* out = nullptr;                             // device [max_jobs][out_stride]
    int* pos = nullptr;                               // device [max_jobs][pos_stride]
    SpeedStreamJob* jobs_dev = nullptr;
    SpeedStreamJob* jobs_host = nullptr;              // page-locked
};

// F(N): the frames decided after N samples of a signal that has not ended: a_k + kSpeedLag <= N  <=>  k * hop * pm <= (N - kSpeedLag + 1) * 1000 - 501
static int64_t speed_frames_ready(int64_t N, int pm) {
    return N < kSpeedLag ? 0 : ((N - kSpeedLag + 1) * 1000 - 501) / ((int64_t)kStretchHop * pm) + 1;
}
int64_t ntts::speed_stream_count_of(int pm, int64_t N, bool last) {
    if (pm == 1000) return N;
    return last ? stretch_len(N, pm) : speed_frames_ready(N, pm) * kStretchHop;
}
// the most one chunk can emit: its last one, which also brings what the lag held back (stream_speed_spec.chunk_out_max)
int64_t ntts::speed_chunk_out_max(int64_t max_chunk_samples, int pm) {
    return pm == 1000 ? max_chunk_samples : stretch_len(max_chunk_samples + kSpeedLag, pm) + 1;
}

void ntts::speed_core_destroy(SpeedStreamCore* k) {
    if (!k) return;
    hipSetDevice(k->c->device);
    hipStreamSynchronize(k->c->stream);
    for (void* b : {(void*)k->hist, (void*)k->state, (void*)k->fade, (void*)k->out, (void*)k->pos, (void*)k->jobs_dev})
        if (b) hipFree(b);
    if (k->jobs_host) hipHostFree(k->jobs_host);
    delete k;
}

int ntts::speed_core_create(ntts_codec* c, int n_streams, int max_chunk_samples, int pm_min, int max_jobs, SpeedStreamCore** out) {
    if (!c || !out) return NTTS_EINVAL;
    if (n_streams < 1) return cfail(c, NTTS_EINVAL, "speed stream: n_streams %d < 1", n_streams);
    if (max_chunk_samples < 1) return cfail(c, NTTS_EINVAL, "speed stream: max_chunk_samples %d < 1", max_chunk_samples);
    if (max_jobs < 1) return cfail(c, NTTS_EINVAL, "speed stream: max_jobs %d < 1", max_jobs);
    if (pm_min < 500 || pm_min > 2000) return cfail(c, NTTS_EINVAL, "speed stream: speed %d per mille outside [500, 2000]", pm_min);
    SpeedStreamCore* k = new SpeedStreamCore();
    k->c = c; k->n = n_streams; k->max_chunk = max_chunk_samples; k->max_jobs = max_jobs;
    k->N.assign(n_streams, 0); k->pm.assign(n_streams, 0); k->parity.assign(n_streams, 0);
    k->out_stride = (long)std::max<int64_t>(max_chunk_samples, speed_chunk_out_max(max_chunk_samples, pm_min < 1000 ? pm_min : 999));
    k->pos_stride = (k->out_stride + kStretchHop - 1) / kStretchHop + 1;
    int rc = NTTS_OK;
#define KHIP(call)                                                                                        \
    do {                                                                                                  \
        hipError_t _s = (call);                                                                           \
        if (_s != hipSuccess) {                                                                           \
            rc = cfail(c, _s == 2 ? NTTS_ENOMEM : NTTS_EHIP, "%s failed: %s", #call, hipGetErrorString(_s)); \
            speed_core_destroy(k);                                                                        \
            return rc;                                                                                    \
        }                                                                                                 \
    } while (0)
    KHIP(hipSetDevice(c->device));
    KHIP(hipMalloc((void**)&k->hist, 2 * (size_t)n_streams * kSpeedHist * sizeof(float)));
    KHIP(hipMemset(k->hist, 0, 2 * (size_t)n_streams * kSpeedHist * sizeof(float)));
    KHIP(hipMalloc((void**)&k->state, (size_t)n_streams * sizeof(SpeedStreamState)));
    KHIP(hipMemset(k->state, 0, (size_t)n_streams * sizeof(SpeedStreamState)));
    {
        std::vector<float> f(kStretchHop);
        for (int i = 0; i < kStretchHop; ++i) f[i] = (float)(0.5 - 0.5 * cos(M_PI * (i + 0.5) / kStretchHop));
        KHIP(hipMalloc((void**)&k->fade, f.size() * sizeof(float)));
        KHIP(hipMemcpy(k->fade, f.data(), f.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    KHIP(hipMalloc((void**)&k->out, (size_t)max_jobs * k->out_stride * sizeof(float)));
    KHIP(hipMemset(k->out, 0, (size_t)max_jobs * k->out_stride * sizeof(float)));
    KHIP(hipMalloc((void**)&k->pos, (size_t)max_jobs * k->pos_stride * sizeof(int)));
    KHIP(hipMemset(k->pos, 0, (size_t)max_jobs * k->pos_stride * sizeof(int)));
    KHIP(hipMalloc((void**)&k->jobs_dev, (size_t)max_jobs * sizeof(SpeedStreamJob)));
    KHIP(hipHostMalloc((void**)&k->jobs_host, (size_t)max_jobs * sizeof(SpeedStreamJob), hipHostMallocDefault));
#undef KHIP
    *out = k;
    return NTTS_OK;
}

long ntts::speed_core_out_stride(const SpeedStreamCore* k) { return k->out_stride; }
long ntts::speed_core_pos_stride(const SpeedStreamCore* k) { return k->pos_stride; }
float* ntts::speed_core_out(const SpeedStreamCore* k) { return k->out; }
int* ntts::speed_core_pos(const SpeedStreamCore* k) { return k->pos; }
int ntts::speed_core_pm(const SpeedStreamCore* k, int u) { return k->pm[u]; }
int64_t ntts::speed_core_total(const SpeedStreamCore* k, int u) { return k->N[u]; }

int64_t ntts::speed_core_peek(const SpeedStreamCore* k, int u, int pm, int n_new, bool last) {
    return speed_stream_count_of(pm, k->N[u] + n_new, last) - speed_stream_count_of(pm, k->N[u], false);
}

int64_t ntts::speed_core_plan(SpeedStreamCore* k, int job, int u, int pm, int n_new, bool last, int phase, int* k0, int* k1) {
    const int64_t N0 = k->N[u], N1 = N0 + n_new;
    const int64_t M0 = speed_stream_count_of(pm, N0, false), M1 = speed_stream_count_of(pm, N1, last);
    SpeedStreamJob& j = k->jobs_host[job];
    j.n_before = (long)N0; j.m0 = (long)M0; j.m1 = (long)M1; j.u = u; j.pm = pm; j.n_new = n_new;
    // (at 1000 the frames that BEGIN in this chunk: their positions are k * hop by definition, host arithmetic of the caller)
    j.k0 = (int)(pm == 1000 ? stretch_frames(N0) : M0 / kStretchHop); j.k1 = (int)stretch_frames(M1);
    j.parity = k->parity[u]; j.last = last ? 1 : 0; j.phase = phase;
    if (k0) *k0 = j.k0;
    if (k1) *k1 = j.k1;
    if (last) { k->N[u] = 0; k->pm[u] = 0; }           // the stream is empty again and may start a new signal, at another speed
    else { k->N[u] = N1; k->pm[u] = pm; }
    if (pm != 1000) k->parity[u] ^= 1;
    return M1 - M0;
}

int ntts::speed_core_run(SpeedStreamCore* k, int n_jobs, const float* in_dev, long in_stride, hipStream_t st) {
    ntts_codec* c = k->c;
    if (n_jobs < 1) return NTTS_OK;
    if (n_jobs > k->max_jobs) return cfail(c, NTTS_EINVAL, "speed stream: %d jobs exceed the %d it was created for", n_jobs, k->max_jobs);
    // The rows are sized for the longest chunk at the slowest speed: checked, not assumed, before anything is written.  The plans have already moved
    // the streams' counts, so a caller must not let this fire: ntts_speed_stream_push refuses an entry above max_chunk_samples before it plans, and
    // a stream set's chunks are at most the out_stride the core was created for (chunk_out_max bounds what either can emit).
    for (int j = 0; j < n_jobs; ++j) {
        const SpeedStreamJob& q = k->jobs_host[j];
        if (q.m1 - q.m0 > k->out_stride || q.n_new > in_stride || q.n_new < 0 || q.k1 - q.k0 > k->pos_stride || q.u < 0 || q.u >= k->n)
            return cfail(c, NTTS_EINVAL, "speed stream: job %d (%d samples in, %ld out, %d frames) exceeds its rows", j, q.n_new, q.m1 - q.m0, q.k1 - q.k0);
    }
    CHIP(c, hipMemcpyAsync(k->jobs_dev, k->jobs_host, (size_t)n_jobs * sizeof(SpeedStreamJob), hipMemcpyHostToDevice, st));
    SpeedStreamArgs a{};
    a.jobs = k->jobs_dev; a.in = in_dev; a.in_stride = in_stride; a.hist = k->hist; a.state = k->state; a.n_streams = k->n; a.fade = k->fade;
    a.out = k->out; a.out_stride = k->out_stride; a.pos = k->pos; a.pos_stride = k->pos_stride;
    // a stream's two jobs of one round depend on each other through its history row and state record: two launches, phase 0 first
    for (int phase = 0; phase < 2; ++phase) {
        int lo = -1, hi = -1;
        for (int j = 0; j < n_jobs; ++j)
            if (k->jobs_host[j].phase == phase) {
                if (lo < 0) lo = j;
                hi = j;
            }
        if (lo < 0) continue;
        NTTS_LAUNCH((wav_stretch_stream_kernel), dim3(hi - lo + 1), dim3(256), st, a, lo, phase);
    }
    return NTTS_OK;
}

// ---- ntts_speed_stream_*: the chunked stretch alone on host chunks, the output format behind it: the streaming twin of ntts_codec_stretch
struct ntts_speed_stream {
    ntts_codec* c = nullptr;
    SpeedStreamCore* k = nullptr;
    WavStreamCore* w = nullptr;          // the output stage behind the stretch; null for 24 kHz float32
    int n = 0, max_chunk = 0;
    float* in_dev = nullptr;             // [n][max_chunk]
    std::vector<int> seen;               // per stream: the call that named it last (repeats within one call)
    std::vector<int> k0, k1, pos_host;
    int call = 0;
    std::string err;
};
static std::string g_speed_stream_err;
extern "C" const char* ntts_speed_stream_last_error(const ntts_speed_stream* ss) { return ss ? ss->err.c_str() : g_speed_stream_err.c_str(); }

extern "C" void ntts_speed_stream_destroy(ntts_speed_stream* ss) {
    if (!ss) return;
    if (ss->w) wav_core_destroy(ss->w);
    if (ss->k) speed_core_destroy(ss->k);
    if (ss->in_dev) hipFree(ss->in_dev);
    delete ss;
}

extern "C" int ntts_speed_stream_create(ntts_codec* c, const ntts_wav_format* fmt, int32_t n_streams, int32_t max_chunk_samples, ntts_speed_stream** out) {
    if (!c || !out) return sfail(g_speed_stream_err, NTTS_EINVAL, "null argument");
    ntts_speed_stream* ss = new ntts_speed_stream();
    ss->c = c; ss->n = n_streams; ss->max_chunk = max_chunk_samples;
    // a stream names its speed with its first chunk: the rows are sized for the slowest one
    int rc = speed_core_create(c, n_streams, max_chunk_samples, 500, n_streams, &ss->k);
    if (rc == NTTS_OK) rc = wav_core_create(c, fmt, n_streams, (int)speed_core_out_stride(ss->k), n_streams, &ss->w);
    if (rc != NTTS_OK) { rc = sfail(g_speed_stream_err, rc, "%s", c->err.c_str()); ntts_speed_stream_destroy(ss); return rc; }
    if (wav_core_plain(ss->w)) { wav_core_destroy(ss->w); ss->w = nullptr; }
    if (hipMalloc((void**)&ss->in_dev, (size_t)n_streams * max_chunk_samples * sizeof(float)) != hipSuccess) {
        (void)hipGetLastError();
        ntts_speed_stream_destroy(ss);
        return sfail(g_speed_stream_err, NTTS_ENOMEM, "speed stream: no device memory for %d x %d samples", n_streams, max_chunk_samples);
    }
    ss->seen.assign(n_streams, 0);
    ss->k0.assign(n_streams, 0); ss->k1.assign(n_streams, 0);
    *out = ss;
    return NTTS_OK;
}

extern "C" int ntts_speed_stream_count(int32_t speed_permille, int64_t n_in_total, int32_t last, int64_t* n_out_total) {
    if (!n_out_total || n_in_total < 0) return sfail(g_speed_stream_err, NTTS_EINVAL, "ntts_speed_stream_count: null / negative argument");
    if (speed_permille < 500 || speed_permille > 2000)
        return sfail(g_speed_stream_err, NTTS_EINVAL, "ntts_speed_stream_count: speed %d per mille outside [500, 2000]", speed_permille);
    *n_out_total = speed_stream_count_of(speed_permille, n_in_total, last != 0);
    return NTTS_OK;
}

extern "C" int ntts_speed_stream_push(ntts_speed_stream* ss, int32_t n, const int32_t* stream, const int32_t* speed_permille, const float* wav,
                                      int64_t in_stride, const int32_t* n_samples, const int32_t* last, void* out, int64_t out_stride, int32_t* out_lens,
                                      int32_t* pos, int64_t pos_stride, int32_t* n_pos) {
    if (!ss) return NTTS_EINVAL;
    std::string& err = ss->err;
    if (n < 1 || !stream || !speed_permille || !wav || !n_samples || !last || !out || !out_lens || in_stride < 0 || (pos && (!n_pos || pos_stride < 0)))
        return sfail(err, NTTS_EINVAL, "null/empty argument");
    // ---- every refusal first: nothing is run and no stream's state moves
    ++ss->call;
    int64_t Lmax = 0, Omax = 0, Kmax = 0;
    bool any = false;
    for (int i = 0; i < n; ++i) {
        const int u = stream[i], pm = speed_permille[i];
        if (u < 0 || u >= ss->n) return sfail(err, NTTS_EINVAL, "entry %d: stream %d outside [0, %d)", i, u, ss->n);
        if (ss->seen[u] == ss->call) return sfail(err, NTTS_EINVAL, "entry %d: stream %d is named twice in one call", i, u);
        ss->seen[u] = ss->call;
        if (n_samples[i] < 0 || n_samples[i] > in_stride)
            return sfail(err, NTTS_EINVAL, "entry %d: n_samples %d outside [0, in_stride %ld]", i, n_samples[i], (long)in_stride);
        if (n_samples[i] > ss->max_chunk) return sfail(err, NTTS_EINVAL, "entry %d: n_samples %d above max_chunk_samples %d", i, n_samples[i], ss->max_chunk);
        if (pm < 500 || pm > 2000) return sfail(err, NTTS_EINVAL, "entry %d: speed %d per mille outside [500, 2000]", i, pm);
        if (speed_core_pm(ss->k, u) && speed_core_pm(ss->k, u) != pm)
            return sfail(err, NTTS_EINVAL, "entry %d: speed %d per mille, but stream %d's signal began at %d: a stream keeps its speed until its last chunk", i,
                          pm, u, speed_core_pm(ss->k, u));
        if (speed_core_total(ss->k, u) + n_samples[i] >= (int64_t)1 << 30)
            return sfail(err, NTTS_EINVAL, "entry %d: stream %d's signal exceeds 2^30 samples", i, u);
        const int64_t s = speed_core_peek(ss->k, u, pm, n_samples[i], last[i] != 0);
        any = any || pm != 1000;
        Lmax = std::max<int64_t>(Lmax, n_samples[i]);
        Omax = std::max(Omax, ss->w ? wav_core_peek(ss->w, u, (int)s, last[i] != 0) : s);
        const int64_t f0 = pm == 1000 ? stretch_frames(speed_core_total(ss->k, u)) : speed_stream_count_of(pm, speed_core_total(ss->k, u), false) / kStretchHop;
        Kmax = std::max(Kmax, stretch_frames(speed_stream_count_of(pm, speed_core_total(ss->k, u) + n_samples[i], last[i] != 0)) - f0);
    }
    if (out_stride < Omax) return sfail(err, NTTS_EINVAL, "out_stride %ld < %ld samples", (long)out_stride, (long)Omax);
    if (pos && pos_stride < Kmax) return sfail(err, NTTS_EINVAL, "pos_stride %ld < %ld frames", (long)pos_stride, (long)Kmax);
    for (int i = 0; i < n; ++i) {
        const int64_t s = speed_core_plan(ss->k, i, stream[i], speed_permille[i], n_samples[i], last[i] != 0, 0, &ss->k0[i], &ss->k1[i]);
        out_lens[i] = (int32_t)(ss->w ? wav_core_plan(ss->w, i, stream[i], (int)s, last[i] != 0, 0) : s);
        if (n_pos) n_pos[i] = ss->k1[i] - ss->k0[i];
    }
    if (pos)                                // unit speed: position k * hop by definition
        for (int i = 0; i < n; ++i)
            for (int k = ss->k0[i]; k < ss->k1[i] && speed_permille[i] == 1000; ++k) pos[(size_t)i * pos_stride + (k - ss->k0[i])] = k * kStretchHop;
    if (!any && !ss->w) {                   // every entry at 1000 in the native format: nothing to compute, nothing is launched
        for (int i = 0; i < n; ++i) memcpy((float*)out + (size_t)i * out_stride, wav + (size_t)i * in_stride, (size_t)n_samples[i] * sizeof(float));
        return NTTS_OK;
    }
    ntts_codec* c = ss->c;
    WHIP(err, hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (Lmax > 0)
        WHIP(err, hipMemcpy2DAsync(ss->in_dev, (size_t)ss->max_chunk * sizeof(float), wav, (size_t)in_stride * sizeof(float), (size_t)Lmax * sizeof(float), n,
                              hipMemcpyHostToDevice, st));
    const float* src = ss->in_dev;          // all at 1000: the stretch is not launched, the chunks go to the output stage as they are
    long src_stride = ss->max_chunk;
    if (any) {
        const int rc = speed_core_run(ss->k, n, ss->in_dev, ss->max_chunk, st);     // (also with no output at all: histories and states move on)
        if (rc != NTTS_OK) return sfail(err, rc, "%s", c->err.c_str());
        src = speed_core_out(ss->k); src_stride = speed_core_out_stride(ss->k);
    }
    size_t esz = sizeof(float);
    const void* res = src;
    long res_stride = src_stride;
    if (ss->w) {
        const int rc = wav_core_run(ss->w, n, src, src_stride, st);
        if (rc != NTTS_OK) return sfail(err, rc, "%s", c->err.c_str());
        esz = wav_core_esz(ss->w); res = wav_core_out(ss->w); res_stride = wav_core_out_stride(ss->w);
    }
    if (Omax > 0)
        WHIP(err, hipMemcpy2DAsync(out, (size_t)out_stride * esz, res, (size_t)res_stride * esz, (size_t)Omax * esz, n, hipMemcpyDeviceToHost, st));
    const long ps = speed_core_pos_stride(ss->k);
    if (pos && any) {
        ss->pos_host.resize((size_t)n * ps);
        WHIP(err, hipMemcpyAsync(ss->pos_host.data(), speed_core_pos(ss->k), (size_t)n * ps * sizeof(int), hipMemcpyDeviceToHost, st));
    }
    WHIP(err, hipStreamSynchronize(st));
    WHIP(err, hipGetLastError());
    if (pos && any)
        for (int i = 0; i < n; ++i)
            if (speed_permille[i] != 1000)
                for (int k = 0; k < ss->k1[i] - ss->k0[i]; ++k) pos[(size_t)i * pos_stride + k] = ss->pos_host[(size_t)i * ps + k];
    return NTTS_OK;
}

extern "C" int ntts_codec_set_cu_mask(ntts_codec* c, const uint32_t* mask, int32_t n_words) {
    if (!c || n_words < 0 || (n_words > 0 && !mask)) return cfail(c, NTTS_EINVAL, "bad CU mask");
    CHIP(c, hipSetDevice(c->device));
    CHIP(c, hipStreamSynchronize(c->stream));
    hipStream_t ns = nullptr;
    if (n_words == 0) CHIP(c, hipStreamCreateWithFlags(&ns, hipStreamNonBlocking));
    else CHIP(c, hipExtStreamCreateWithCUMask(&ns, (uint32_t)n_words, mask));
    const bool lent = c->stream != c->own_stream;       // (a stream lent by the caller stays in use; the mask applies to the engine's own)
    hipStreamDestroy(c->own_stream);
    c->own_stream = ns;
    if (!lent) c->stream = ns;
    return NTTS_OK;
}

// The codec passes on a stream of the caller's; nullptr returns to the engine's own.  Blocking: drains the stream in use.
extern "C" int ntts_codec_set_stream(ntts_codec* c, void* stream) {
    if (!c) return NTTS_EINVAL;
    CHIP(c, hipSetDevice(c->device));
    CHIP(c, hipStreamSynchronize(c->stream));
    c->stream = stream ? (hipStream_t)stream : c->own_stream;
    return NTTS_OK;
}

extern "C" int ntts_codec_sync(ntts_codec* c) {
    if (!c) return NTTS_EINVAL;
    CHIP(c, hipSetDevice(c->device));
    // On a stream the caller lent, wait for the codec's own most recent pass only: the caller may have enqueued a whole decode phase
    // behind it on the same stream (bench.py's lanes), which is none of this call's business.
    if (c->stream != c->own_stream && c->have_done) CHIP(c, hipEventSynchronize(c->ev_done));
    else CHIP(c, hipStreamSynchronize(c->stream));
    CHIP(c, hipGetLastError());
    return NTTS_OK;
}

// Test tap: keep the fp32 residual stream after the four stages of hf:models/xcodec2/modeling_xcodec2.py:838-862 -- 0 embed (fc + k = 7 conv),
// 1 prior_net (2 ResNet blocks), 2 the transformer layers, 3 post_net (2 ResNet blocks) -- of the most recent decode call.
extern "C" int ntts_codec_set_debug(ntts_codec* c, int32_t keep_stages) {
    if (!c) return NTTS_EINVAL;
    CHIP(c, hipSetDevice(c->device));
    CHIP(c, hipStreamSynchronize(c->stream));
    if (keep_stages && !c->tap) {
        CHIP(c, hipMalloc((void**)&c->tap, 4 * (size_t)c->max_rows * c->H * sizeof(float)));
        CHIP(c, hipMemset(c->tap, 0, 4 * (size_t)c->max_rows * c->H * sizeof(float)));
    } else if (!keep_stages && c->tap) {
        CHIP(c, hipFree(c->tap));
        c->tap = nullptr;
    }
    c->tap_off.clear(); c->tap_len.clear();
    return NTTS_OK;
}
extern "C" int ntts_codec_read_stage(ntts_codec* c, int32_t stage, int32_t utt, float* out, int64_t cap, int32_t* rows, int32_t* cols) {
    if (!c || !out || !rows || !cols || stage < 0 || stage > 3) return cfail(c, NTTS_EINVAL, "bad argument");
    if (!c->tap || utt < 0 || utt >= (int)c->tap_len.size()) return cfail(c, NTTS_ESTATE, "no stage outputs kept for utterance %d: ntts_codec_set_debug(c, 1), then decode", utt);
    const long need = (long)c->tap_len[utt] * c->H;
    if (cap < need) return cfail(c, NTTS_EINVAL, "stage output needs %ld floats", need);
    CHIP(c, hipSetDevice(c->device));
    CHIP(c, hipStreamSynchronize(c->stream));
    CHIP(c, hipMemcpy(out, c->tap + ((size_t)stage * c->max_rows + c->tap_off[utt] + kPadRows) * c->H, (size_t)need * sizeof(float), hipMemcpyDeviceToHost));
    *rows = c->tap_len[utt];
    *cols = c->H;
    return NTTS_OK;
}

extern "C" int ntts_codec_stream(ntts_codec* c, void** stream) {
    if (!c || !stream) return NTTS_EINVAL;
    *stream = (void*)c->stream;
    return NTTS_OK;
}
extern "C" int ntts_codec_limits(ntts_codec* c, int32_t* max_frames, int64_t* max_rows) {
    if (!c || !max_frames || !max_rows) return NTTS_EINVAL;
    *max_frames = c->cfg.max_frames;
    *max_rows = c->max_rows;
    return NTTS_OK;
}

extern "C" int ntts_host_alloc(size_t bytes, void** out) {
    if (!out || bytes == 0) return NTTS_EINVAL;
    return hipHostMalloc(out, bytes, hipHostMallocDefault) == hipSuccess ? NTTS_OK : NTTS_ENOMEM;
}
extern "C" int ntts_host_free(void* p) { return (!p || hipHostFree(p) == hipSuccess) ? NTTS_OK : NTTS_EHIP; }

// A plain non-blocking HIP stream on `device` for callers without a runtime of their own (neutts._hip.EngineGang: the lanes
// several engines' decode chains and the shared matrix-pass stream run on).  Streams created back to back land in different
// hardware queues (the runtime assigns the least-loaded of its four).
extern "C" int ntts_stream_create(int32_t device, void** stream) {
    if (!stream) return NTTS_EINVAL;
    hipStream_t st = nullptr;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) {
        (void)hipGetLastError();
        return NTTS_EHIP;
    }
    *stream = (void*)st;
    return NTTS_OK;
}
extern "C" int ntts_stream_destroy(int32_t device, void* stream) {
    if (!stream) return NTTS_OK;
    if (hipSetDevice(device) != hipSuccess || hipStreamSynchronize((hipStream_t)stream) != hipSuccess || hipStreamDestroy((hipStream_t)stream) != hipSuccess) {
        (void)hipGetLastError();
        return NTTS_EHIP;
    }
    return NTTS_OK;
}

extern "C" int ntts_codec_last_timing(ntts_codec* c, float* ms) {
    if (!c || !ms) return NTTS_EINVAL;
    *ms = 0;
    if (c->have_time) CHIP(c, hipEventElapsedTime(ms, c->ev[0], c->ev[1]));
    return NTTS_OK;
}
