// resnet.cpp -- forward pass of the ResNet18 classifier used by the reference's explainability passes
// (xai/XAI.py:357-471: torchvision resnet18 with fc -> num_classes, eval mode).
//
// BatchNorm (eval) is folded into the preceding convolution at load time, in float64:
//     w' = w * gamma / sqrt(var + eps),   b' = beta - mean * gamma / sqrt(var + eps)
// so every conv+BN(+ReLU)(+identity) is ONE launch of conv_mfma_kernel with its bias / residual / ReLU
// epilogue.  The pre-processing of XAI.py:399-431 is one fused kernel (classifier.hip).
//
// Training (the second half of this file), BatchNorm frozen: the training forward is this forward, the backward pass is
// the data-gradient walk of sisic_resnet_input_gradient with a weight gradient issued at every convolution, and after the
// Adam step the folded filters are derived again on the device from the un-folded parameters.
// Training with batch statistics (an option of the same forward and the same walk): every convolution runs with its UNFOLDED
// filters and is followed by the BatchNorm launches of batchnorm.hip; the walk gains a BatchNorm backward in front of every
// weight gradient, gamma and beta train, the running statistics follow the batches, and every optimizer step derives the
// folded inference forms again from (w, gamma, beta, running_mean, running_var) with the load path's arithmetic.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>

#include "common.h"
#include "train.h"
#include "workspace.h"

using namespace sisic;

namespace {

struct FoldedConv {
    int cout = 0, cin = 0, k = 0, stride = 1;
    int w_idx = -1;
    int bn_w = -1, bn_b = -1, bn_m = -1, bn_v = -1;
    float* packed = nullptr;
    float* wino = nullptr;           // Winograd-domain filters of the BN-folded weight (3x3 stride 1 only)
    float* bias = nullptr;
    // backward-to-input (sisic_resnet_input_gradient): the same convolution with transposed, tap-flipped filters
    float* raw = nullptr;            // BN-folded OIHW weight on the device (the stem's transposed convolution reads it)
    float* raw_t = nullptr;          // its transposed, tap-flipped copy [cin][cout][k*k] (not for the 7x7 stem)
    double* sc = nullptr;            // BatchNorm scale gamma / sqrt(var + eps) per output channel, in double (sisic_resnet_randomize)
    float* packed_t = nullptr;       // packed [cout -> cin] filters W'[ci][co][a][b] = W[co][ci][k-1-a][k-1-b]
    float* wino_t = nullptr;         // their Winograd form (3x3 stride 1 only)
    // batch-statistics training only (sisic_resnet_train_begin_bn, mode 1; NULL otherwise): the same forms of the UNFOLDED
    // weight, which itself lives in the parameter arena.  The 7x7 stem has the packed form alone.
    struct Plain {
        float* raw_t = nullptr;
        float* packed = nullptr;
        float* wino = nullptr;
        float* packed_t = nullptr;
        float* wino_t = nullptr;
    } u;
};

struct Block {
    FoldedConv conv1, conv2, down;   // down.k == 0 when the shortcut is the identity
};

// sisic_resnet_train_begin .. train_end: the 22 trainable tensors un-folded, side by side in one arena (each at a multiple of
// four floats; the padding stays zero in all four arenas), so that the statistics and the Adam pass are one launch each
struct ResnetTrain {
    std::vector<int64_t> off;        // arena offset of tensor i (sisic_resnet_tensor_name order), -1: frozen (BatchNorm)
    size_t floats = 0;
    float* param = nullptr;
    float* grad = nullptr;
    float* adam_m = nullptr;
    float* adam_v = nullptr;
    float* part = nullptr;           // K-split partial slabs of the weight gradients
    size_t part_floats = 0;
    void* stats = nullptr;           // GradStats record, the loss (at byte 12), then the statistics scratch (at byte 16)
    // every packed and Winograd form of the 19 filters behind the stem, rebuilt after a step by two batched launches
    // (repack.hip: the jobs carry the arithmetic of launch_conv_pack / launch_winograd_pack): the first layouts from raw and
    // raw_t, then the Winograd layouts that are derived from the first one
    void* repack_dev[2] = {nullptr, nullptr};
    int repack_jobs[2] = {0, 0}, repack_blocks[2] = {0, 0};
    std::vector<int> labels_host;    // staging of the labels and the class weights of a call
    std::vector<float> cw_host;
    int64_t step = 0;
    // batch-statistics BatchNorm (bn_mode 1): gamma and beta have offsets in `off` like every trainable tensor; the 40 running
    // statistics live in a buffer arena of their own (boff: offset, -1 for everything else)
    int bn_mode = 0;
    double momentum = 0.1;
    std::vector<int64_t> boff;
    size_t buf_floats = 0;
    float* buf = nullptr;
    bool stats_moved = false;        // a loss_backward updated the running statistics after the folded forms were last derived
    std::vector<float*> plain_owned; // the second set of filter forms (FoldedConv::u)
    // the unfolded forms, rebuilt by three batched launches: raw_t / packed / first Winograd layout from the arena, then what
    // reads those, then the Winograd layouts of the transposed filters
    void* plain_dev[3] = {nullptr, nullptr, nullptr};
    int plain_jobs[3] = {0, 0, 0}, plain_blocks[3] = {0, 0, 0};
};

}  // namespace

struct sisic_resnet {
    sisic_ctx* ctx = nullptr;
    int num_classes = 0;
    TensorDir dir;                          // expected state dict
    std::vector<std::vector<float>> host;   // host copies (folding happens on the host)
    FoldedConv stem;
    std::vector<Block> blocks;
    int fc_w = -1, fc_b = -1;
    float* d_fc_w = nullptr;
    float* d_fc_b = nullptr;
    std::vector<float*> owned;
    Pool pool;
    int ws_B = 0, ws_H = 0, ws_W = 0;       // shape the pooled blocks were sized for (see workspace_for)
    // renewed whenever pooled blocks or weight buffers are released or derived again: a captured sampling step that ran the
    // input-gradient walk (sisic_sample_frames_clf) holds their addresses and is re-captured when this has moved.  Every value
    // comes from one process-wide counter (next_workspace_generation), so no two states of any two handles share one: a
    // handle destroyed and created again at the same address never matches a key the old one left behind.
    uint64_t ws_gen = 0;
    // sisic_resnet_input_gradient_targets: the call's targets as ints, in a pinned ring; a slot is written again only after
    // the copy out of it has finished (its event), so the call does not wait for its stream
    static constexpr int TARGET_SLOTS = 4;
    int* targets_stage = nullptr;
    size_t targets_cap = 0;
    uint64_t targets_next = 0;
    hipEvent_t targets_ev[TARGET_SLOTS] = {};
    bool targets_used[TARGET_SLOTS] = {};
    bool loaded = false;
    ResnetTrain* train = nullptr;
};

namespace {

constexpr float BN_EPS = 1e-5f;   // torchvision BatchNorm2d default

// the next value of sisic_resnet::ws_gen, unique in the process
uint64_t next_workspace_generation() {
    static std::atomic<uint64_t> counter{0};
    return counter.fetch_add(1) + 1;
}

// targets (host int64, already checked) as ints in dst, ordered on s, through the handle's pinned ring
int stage_targets(sisic_resnet* r, const int64_t* targets, int B, int* dst, hipStream_t s) {
    if (r->targets_cap < (size_t)B) {
        SISIC_HIP(hipDeviceSynchronize());
        if (r->targets_stage) SISIC_HIP(hipHostFree(r->targets_stage));
        r->targets_stage = nullptr;
        const size_t cap = std::max<size_t>((size_t)B, 256);
        void* p = nullptr;
        SISIC_HIP(hipHostMalloc(&p, cap * sisic_resnet::TARGET_SLOTS * sizeof(int), hipHostMallocDefault));
        r->targets_stage = static_cast<int*>(p);
        r->targets_cap = cap;
        for (bool& used : r->targets_used) used = false;
    }
    const int slot = (int)(r->targets_next++ % sisic_resnet::TARGET_SLOTS);
    if (!r->targets_ev[slot]) SISIC_HIP(hipEventCreateWithFlags(&r->targets_ev[slot], hipEventDisableTiming));
    if (r->targets_used[slot]) SISIC_HIP(hipEventSynchronize(r->targets_ev[slot]));
    int* h = r->targets_stage + (size_t)slot * r->targets_cap;
    for (int b = 0; b < B; ++b) h[b] = (int)targets[b];
    SISIC_HIP(hipMemcpyAsync(dst, h, (size_t)B * sizeof(int), hipMemcpyHostToDevice, s));
    SISIC_HIP(hipEventRecord(r->targets_ev[slot], s));
    r->targets_used[slot] = true;
    return SISIC_OK;
}

void add_conv_bn(sisic_resnet* r, FoldedConv& c, const std::string& conv, const std::string& bn, int cout, int cin, int k,
                 int stride) {
    c.cout = cout; c.cin = cin; c.k = k; c.stride = stride;
    c.w_idx = r->dir.add(conv + ".weight", (int64_t)cout * cin * k * k);
    c.bn_w = r->dir.add(bn + ".weight", cout);
    c.bn_b = r->dir.add(bn + ".bias", cout);
    c.bn_m = r->dir.add(bn + ".running_mean", cout);
    c.bn_v = r->dir.add(bn + ".running_var", cout);
}

void describe(sisic_resnet* r) {
    r->dir.noun = "float tensors";              // (num_batches_tracked, an integer tensor of the state dict, never comes here)
    const std::string pre = "model.";           // XAI.py:389: self.model = models.resnet18(...)
    add_conv_bn(r, r->stem, pre + "conv1", pre + "bn1", 64, 3, 7, 2);
    const int widths[4] = {64, 128, 256, 512};
    int in_ch = 64;
    for (int l = 0; l < 4; ++l) {
        for (int j = 0; j < 2; ++j) {
            Block b;
            const int stride = (l > 0 && j == 0) ? 2 : 1;
            const std::string base = pre + "layer" + std::to_string(l + 1) + "." + std::to_string(j);
            add_conv_bn(r, b.conv1, base + ".conv1", base + ".bn1", widths[l], in_ch, 3, stride);
            add_conv_bn(r, b.conv2, base + ".conv2", base + ".bn2", widths[l], widths[l], 3, 1);
            if (stride != 1 || in_ch != widths[l])
                add_conv_bn(r, b.down, base + ".downsample.0", base + ".downsample.1", widths[l], in_ch, 1, stride);
            r->blocks.push_back(b);
            in_ch = widths[l];
        }
    }
    r->fc_w = r->dir.add(pre + "fc.weight", (int64_t)r->num_classes * 512);
    r->fc_b = r->dir.add(pre + "fc.bias", r->num_classes);
}

int dev_alloc(sisic_resnet* r, size_t floats, float** out) {
    void* p = nullptr;
    SISIC_HIP(hipMalloc(&p, std::max<size_t>(floats, 4) * sizeof(float)));
    SISIC_TRY(poison_fresh(p, std::max<size_t>(floats, 4) * sizeof(float)));
    r->owned.push_back(static_cast<float*>(p));
    *out = static_cast<float*>(p);
    return SISIC_OK;
}

// BatchNorm scale of output channel co in double: gamma / sqrt(var + eps)
inline double bn_scale(const sisic_resnet* r, const FoldedConv& c, int co) {
    return (double)r->host[c.bn_w][co] / std::sqrt((double)r->host[c.bn_v][co] + (double)BN_EPS);
}

// every device buffer of one convolution (once per sisic_resnet_load; nothing below allocates)
int fold_alloc(sisic_resnet* r, FoldedConv& c) {
    if (c.k == 0) return SISIC_OK;
    const size_t numel = (size_t)c.cout * c.cin * c.k * c.k;
    SISIC_TRY(dev_alloc(r, numel, &c.raw));
    SISIC_TRY(dev_alloc(r, (size_t)sisic_conv_packed_numel(c.cout, c.cin, c.k), &c.packed));
    if (c.k == 3 && c.stride == 1)       // F(2x2,3x3) for the 13 stride-1 3x3 convolutions (conv_winograd.hip)
        SISIC_TRY(dev_alloc(r, (size_t)winograd_packed_numel(c.cout, c.cin), &c.wino));
    SISIC_TRY(dev_alloc(r, c.cout, &c.bias));
    float* sc = nullptr;
    SISIC_TRY(dev_alloc(r, 2 * (size_t)c.cout, &sc));        // cout doubles (hipMalloc aligns to 256 bytes)
    c.sc = reinterpret_cast<double*>(sc);
    if (c.k != 7) {                      // backward filters (the 7x7 stem has its own kernel, classifier_bwd.hip)
        SISIC_TRY(dev_alloc(r, numel, &c.raw_t));
        SISIC_TRY(dev_alloc(r, (size_t)sisic_conv_packed_numel(c.cin, c.cout, c.k), &c.packed_t));
        if (c.k == 3 && c.stride == 1) SISIC_TRY(dev_alloc(r, (size_t)winograd_packed_numel(c.cin, c.cout), &c.wino_t));
    }
    return SISIC_OK;
}

// packed / Winograd forms of raw and raw_t, into the buffers the handle owns
int fold_pack(sisic_resnet* r, FoldedConv& c, hipStream_t s) {
    if (c.k == 0) return SISIC_OK;
    SISIC_TRY(launch_conv_pack(r->ctx, c.raw, c.cout, c.cin, c.k, c.packed, s));
    if (c.wino) SISIC_TRY(launch_winograd_pack(r->ctx, c.raw, c.cout, c.cin, c.wino, s));
    if (c.raw_t) {
        SISIC_TRY(launch_conv_pack(r->ctx, c.raw_t, c.cin, c.cout, c.k, c.packed_t, s));
        if (c.wino_t) SISIC_TRY(launch_winograd_pack(r->ctx, c.raw_t, c.cin, c.cout, c.wino_t, s));
    }
    return SISIC_OK;
}

// the loaded weight (r->host) folded on the host in float64 and uploaded, then every derived form (sisic_resnet_load and
// sisic_resnet_restore).  The copies are blocking: the host vectors are locals.
int fold(sisic_resnet* r, FoldedConv& c, hipStream_t s) {
    if (c.k == 0) return SISIC_OK;
    const std::vector<float>& w = r->host[c.w_idx];
    const std::vector<float>& be = r->host[c.bn_b];
    const std::vector<float>& m = r->host[c.bn_m];
    const size_t per = (size_t)c.cin * c.k * c.k;
    std::vector<float> wf(w.size()), bf(c.cout);
    std::vector<double> scv(c.cout);
    for (int co = 0; co < c.cout; ++co) {
        const double sc = bn_scale(r, c, co);
        scv[co] = sc;
        for (size_t i = 0; i < per; ++i) wf[co * per + i] = (float)((double)w[co * per + i] * sc);
        bf[co] = (float)((double)be[co] - (double)m[co] * sc);
    }
    SISIC_HIP(hipMemcpy(c.raw, wf.data(), wf.size() * sizeof(float), hipMemcpyHostToDevice));
    SISIC_HIP(hipMemcpy(c.bias, bf.data(), bf.size() * sizeof(float), hipMemcpyHostToDevice));
    SISIC_HIP(hipMemcpy(c.sc, scv.data(), scv.size() * sizeof(double), hipMemcpyHostToDevice));
    if (c.raw_t) {
        const int kk = c.k * c.k;
        std::vector<float> wt(wf.size());
        for (int co = 0; co < c.cout; ++co)
            for (int ci = 0; ci < c.cin; ++ci)
                for (int t = 0; t < kk; ++t)
                    wt[((size_t)ci * c.cout + co) * kk + (kk - 1 - t)] = wf[((size_t)co * c.cin + ci) * kk + t];
        SISIC_HIP(hipMemcpy(c.raw_t, wt.data(), wt.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    return fold_pack(r, c, s);
}

// fold() of every convolution and the fc weight: the device state of the loaded, un-randomised model
int derive_from_host(sisic_resnet* r, hipStream_t s) {
    SISIC_TRY(fold(r, r->stem, s));
    for (auto& b : r->blocks) {
        SISIC_TRY(fold(r, b.conv1, s));
        SISIC_TRY(fold(r, b.conv2, s));
        SISIC_TRY(fold(r, b.down, s));
    }
    SISIC_HIP(hipMemcpy(r->d_fc_w, r->host[r->fc_w].data(), r->host[r->fc_w].size() * sizeof(float), hipMemcpyHostToDevice));
    SISIC_HIP(hipMemcpy(r->d_fc_b, r->host[r->fc_b].data(), r->host[r->fc_b].size() * sizeof(float), hipMemcpyHostToDevice));
    return SISIC_OK;
}

// The pool matches blocks by exact size, so every distinct (batch, resolution) would leave its own full set of
// activation buffers behind (the stem output alone is B*64*112*112*4 bytes).  Like the UNet's check_shape, the pool is
// therefore emptied whenever the input shape changes: resident workspace = what the current shape needs, whatever the
// history of batch sizes (trajectory lengths, last chunks of Integrated Gradients, ...) has been.
int workspace_for(sisic_resnet* r, int B, int H, int W) {
    if (r->ws_B == B && r->ws_H == H && r->ws_W == W) return SISIC_OK;
    SISIC_HIP(hipDeviceSynchronize());       // earlier launches may still use the blocks
    r->pool.release_all();
    r->ws_gen = next_workspace_generation();
    r->ws_B = B; r->ws_H = H; r->ws_W = W;
    return SISIC_OK;
}

// What every entry point that runs the network starts with, behind its own argument checks.
int begin_run(sisic_resnet* r, const char* who, int B, int H, int W) {
    if (!r->loaded) {
        set_error("%s called before sisic_resnet_load", who);
        return SISIC_ESTATE;
    }
    SISIC_HIP(hipSetDevice(r->ctx->device));
    return workspace_for(r, B, H, W);
}

// The filter forms one launch reads: the BatchNorm-folded set with its bias, or (batch-statistics training) the forms of the
// unfolded weight, which has no bias because its BatchNorm follows.  A view; the buffers stay with the FoldedConv.
struct ConvForms {
    const float* packed;
    const float* wino;
    const float* packed_t;
    const float* wino_t;
    const float* bias;
};

ConvForms forms_of(const FoldedConv& c, bool plain) {
    if (plain) return {c.u.packed, c.u.wino, c.u.packed_t, c.u.wino_t, nullptr};
    return {c.packed, c.wino, c.packed_t, c.wino_t, c.bias};
}

int conv_fwd(sisic_resnet* r, const FoldedConv& c, const ConvForms& f, const float* in, int B, int H, int W, const float* residual,
             bool relu, float* out, hipStream_t s) {
    sisic_conv_args a{};
    a.in0 = in; a.c0 = c.cin; a.B = B; a.Hin = H; a.Win = W;
    a.ksize = c.k; a.stride = c.stride;
    a.w_packed = f.packed; a.bias = f.bias; a.Cout = c.cout;
    a.w_winograd = f.wino;
    a.residual = residual; a.relu = relu ? 1 : 0; a.out = out;
    return launch_conv2d(r->ctx, a, s);
}

// transposed convolution of `c` applied to g [B, c.cout, gh, gw]; stride 2: zero-insertion input (2gh x 2gw grid)
int conv_t(sisic_resnet* r, const FoldedConv& c, const ConvForms& f, const float* g, int B, int gh, int gw, const float* residual,
           float* out, hipStream_t s) {
    sisic_conv_args a{};
    a.in0 = g; a.c0 = c.cout; a.B = B; a.Hin = gh; a.Win = gw;
    a.ksize = c.k; a.stride = 1;
    a.upsample = (c.k == 3 && c.stride == 2) ? 2 : 0;
    a.w_packed = f.packed_t; a.w_winograd = f.wino_t; a.Cout = c.cin;
    a.residual = residual; a.out = out;
    return launch_conv2d(r->ctx, a, s);
}

inline int out_dim(int n, int k, int stride) { return (n + 2 * (k / 2) - k) / stride + 1; }

// training: tensor idx in the parameter and gradient arenas, and (batch statistics) in the arena of the running statistics
float* param_of(ResnetTrain* tr, int idx) { return tr->param + tr->off[idx]; }
float* grad_of(ResnetTrain* tr, int idx) { return tr->grad + tr->off[idx]; }
float* stat_of(ResnetTrain* tr, int idx) { return tr->buf + tr->boff[idx]; }

// what the training forward keeps of one BatchNorm: the convolution's output y and (mean, invstd, var) [3][C]
struct BnKept {
    float* y = nullptr;
    float* st = nullptr;
    int C = 0, HW = 0;
};

// The forward pass every entry point below runs: [pre-processing ->] stem -> max-pool -> the 8 blocks -> avgpool + fc.
// Options in, what the caller goes on with out.  Every activation is a block of the caller's scope; what no option keeps
// goes back to the pool as soon as its last reader has been launched.
struct Trunk {
    bool preprocess = true;
    float* stem_out = nullptr;   // stop after the stem, which writes here (sisic_resnet_stem)
    bool keep = false;           // keep c1, the max-pool output and every block's t1 and output (the input gradient reads them)
    bool keep_pre = false;       // keep the pre-processed input as well (the stem's weight gradient reads it)
    // train with batch statistics (implies keep and keep_pre): every convolution step is conv (unfolded filters, no bias) ->
    // moments (which also move the running statistics) -> apply, its y and moments kept; the head reads fc from the arena
    ResnetTrain* bn = nullptr;
    float* pre = nullptr;        // keep_pre with preprocess: the stem's input [B, 3, 224, 224]
    const char* who = "resnet_input_gradient";
    bool split_last = false;     // last block: bn2(conv2(.)) alone into ylast, then relu(. + identity) (Grad-CAM reads ylast)
    float* logits = nullptr;     // where the logits go; nullptr: into a block of the scope, returned here
    float* features = nullptr;   // stop at the pooled features [B, 512], written here: no Linear, no logits (sisic_resnet_features)
    struct Saved { float* t1; float* out; int h, w, bh, bw; BnKept k1, k2, kd; };
    std::vector<Saved> saved;    // keep: one per block
    BnKept stem_k;               // bn: the stem's BatchNorm
    float* c1 = nullptr;         // relu(bn1(conv1(.))) [B, 64, c1h, c1w]
    float* m = nullptr;          // its max-pool
    int c1h = 0, c1w = 0;
    float* act = nullptr;        // the last block's output [B, 512, h, w]
    float* ylast = nullptr;
    int h = 0, w = 0;
};

// One convolution step of the trunk: out = [relu](conv(in) [+ residual]) with the folded filters and their bias in one launch.
// t.bn: out = [relu](bn(conv(in)) [+ residual]) with the unfolded filters and the batch's statistics, y and the moments kept in k.
int conv_step(sisic_resnet* r, PoolScope& ws, const Trunk& t, const FoldedConv& c, const float* in, int B, int h, int w,
              const float* residual, bool relu, float* out, BnKept& k, hipStream_t s) {
    if (!t.bn) return conv_fwd(r, c, forms_of(c, false), in, B, h, w, residual, relu, out, s);
    k.C = c.cout; k.HW = out_dim(h, c.k, c.stride) * out_dim(w, c.k, c.stride);
    SISIC_TRY(ws.get((size_t)B * k.C * k.HW, &k.y));
    SISIC_TRY(ws.get(3 * (size_t)k.C, &k.st));
    SISIC_TRY(conv_fwd(r, c, forms_of(c, true), in, B, h, w, nullptr, false, k.y, s));
    SISIC_TRY(launch_bn_moments(r->ctx, k.y, B, k.C, k.HW, BN_EPS, k.st, k.st + k.C, k.st + 2 * k.C, stat_of(t.bn, c.bn_m),
                                stat_of(t.bn, c.bn_v), t.bn->momentum, s));
    return launch_bn_apply(r->ctx, k.y, param_of(t.bn, c.bn_w), param_of(t.bn, c.bn_b), k.st, k.st + k.C, residual, relu, out, B, k.C,
                           k.HW, s);
}

int run_trunk(sisic_resnet* r, PoolScope& ws, const float* x, int B, int H, int W, Trunk& t, hipStream_t s) {
    if (t.bn) {
        t.keep = t.keep_pre = true;
        t.bn->stats_moved = true;
    }
    const float* cur = x;
    int h = H, w = W;
    float* pre = nullptr;
    if (t.preprocess) {
        const int S = 224;                      // CLASSIFIER_IMAGE_SIZE, XAI.py
        SISIC_TRY(ws.get((size_t)B * 3 * S * S, &pre));
        SISIC_TRY(launch_preprocess(r->ctx, x, pre, B, H, W, S, S, s));
        cur = pre; h = S; w = S;
    }
    // stem: conv7x7 s2 (+BN) + ReLU, maxpool 3x3 s2
    t.c1h = out_dim(h, 7, 2); t.c1w = out_dim(w, 7, 2);
    t.c1 = t.stem_out;
    if (!t.c1) SISIC_TRY(ws.get((size_t)B * 64 * t.c1h * t.c1w, &t.c1));
    SISIC_TRY(conv_step(r, ws, t, r->stem, cur, B, h, w, nullptr, true, t.c1, t.stem_k, s));
    if (pre && t.keep_pre) t.pre = pre;
    else if (pre) ws.put(pre);
    if (t.stem_out) return SISIC_OK;
    h = t.c1h; w = t.c1w;
    if (t.keep) SISIC_REQUIRE(h % 2 == 0 && w % 2 == 0, "%s: odd feature map", t.who);
    const int mh = out_dim(h, 3, 2), mw = out_dim(w, 3, 2);
    SISIC_TRY(ws.get((size_t)B * 64 * mh * mw, &t.m));
    SISIC_TRY(launch_maxpool(r->ctx, t.c1, t.m, B, 64, h, w, s));
    if (!t.keep) ws.put(t.c1);
    float* act = t.m;
    h = mh; w = mw;
    for (const Block& b : r->blocks) {
        const bool split = t.split_last && &b == &r->blocks.back();
        const int bh = out_dim(h, 3, b.conv1.stride), bw = out_dim(w, 3, b.conv1.stride);
        if (t.keep)
            SISIC_REQUIRE(b.conv1.stride == 1 || (h % 2 == 0 && w % 2 == 0), "%s: odd feature map %dx%d", t.who, h, w);
        BnKept k1, k2, kd;
        float* t1 = nullptr;
        SISIC_TRY(ws.get((size_t)B * b.conv1.cout * bh * bw, &t1));
        SISIC_TRY(conv_step(r, ws, t, b.conv1, act, B, h, w, nullptr, true, t1, k1, s));
        const float* identity = act;
        float* ds = nullptr;
        if (b.down.k) {
            SISIC_TRY(ws.get((size_t)B * b.down.cout * bh * bw, &ds));
            SISIC_TRY(conv_step(r, ws, t, b.down, act, B, h, w, nullptr, false, ds, kd, s));
            identity = ds;
        }
        float* t2 = nullptr;
        const size_t n_out = (size_t)B * b.conv2.cout * bh * bw;
        SISIC_TRY(ws.get(n_out, &t2));
        if (!split) {
            SISIC_TRY(conv_step(r, ws, t, b.conv2, t1, B, bh, bw, identity, true, t2, k2, s));    // relu(bn2(conv2) + identity)
        } else {
            SISIC_TRY(ws.get(n_out, &t.ylast));
            SISIC_TRY(conv_step(r, ws, t, b.conv2, t1, B, bh, bw, nullptr, false, t.ylast, k2, s));
            SISIC_TRY(launch_add_relu(r->ctx, t.ylast, identity, t2, (int64_t)n_out, s));
        }
        if (ds) ws.put(ds);
        if (t.keep) {
            t.saved.push_back({t1, t2, h, w, bh, bw, k1, k2, kd});
        } else {
            ws.put(t1);
            ws.put(act);
        }
        act = t2; h = bh; w = bw;
    }
    if (t.features) {
        SISIC_TRY(launch_avgpool(r->ctx, act, t.features, B, r->blocks.back().conv2.cout, h * w, s));
        t.act = act; t.h = h; t.w = w;
        return SISIC_OK;
    }
    if (!t.logits) SISIC_TRY(ws.get((size_t)B * r->num_classes, &t.logits));
    const float* fc_w = t.bn ? param_of(t.bn, r->fc_w) : r->d_fc_w;
    const float* fc_b = t.bn ? param_of(t.bn, r->fc_b) : r->d_fc_b;
    SISIC_TRY(launch_avgpool_fc(r->ctx, act, fc_w, fc_b, t.logits, B, r->blocks.back().conv2.cout, h * w, r->num_classes, s));
    t.act = act; t.h = h; t.w = w;
    return SISIC_OK;
}

// the training arenas (the caller has synchronised the device)
void train_free(sisic_resnet* r) {
    ResnetTrain* tr = r->train;
    if (!tr) return;
    for (float* p : {tr->param, tr->grad, tr->adam_m, tr->adam_v, tr->part}) (void)hipFree(p);
    (void)hipFree(tr->stats);
    for (void* p : tr->repack_dev) (void)hipFree(p);
    (void)hipFree(tr->buf);
    for (void* p : tr->plain_dev) (void)hipFree(p);
    for (float* p : tr->plain_owned) (void)hipFree(p);
    auto forget = [](FoldedConv& c) { c.u = FoldedConv::Plain(); };
    forget(r->stem);
    for (auto& b : r->blocks) { forget(b.conv1); forget(b.conv2); forget(b.down); }
    delete tr;
    r->train = nullptr;
}

}  // namespace

extern "C" {

int sisic_resnet_create(sisic_ctx* ctx, int num_classes, sisic_resnet** out) {
    SISIC_REQUIRE(ctx && out && num_classes > 0 && num_classes <= 1000, "resnet_create: bad arguments");
    auto* r = new sisic_resnet();
    r->ctx = ctx;
    r->num_classes = num_classes;
    r->ws_gen = next_workspace_generation();
    describe(r);
    *out = r;
    return SISIC_OK;
}

int sisic_resnet_destroy(sisic_resnet* r) {
    if (!r) return SISIC_OK;
    (void)hipDeviceSynchronize();
    train_free(r);
    for (auto p : r->owned) (void)hipFree(p);
    r->pool.release_all();
    if (r->targets_stage) (void)hipHostFree(r->targets_stage);
    for (auto e : r->targets_ev)
        if (e) (void)hipEventDestroy(e);
    delete r;
    return SISIC_OK;
}

int64_t sisic_resnet_workspace_bytes(const sisic_resnet* r) {
    return r ? r->pool.bytes() : 0;
}

int sisic_resnet_num_tensors(const sisic_resnet* r) { return r ? r->dir.size() : 0; }

const char* sisic_resnet_tensor_name(const sisic_resnet* r, int i) { return r ? r->dir.name(i) : nullptr; }

int sisic_resnet_load(sisic_resnet* r, int n, const char* const* names, const float* const* host_ptrs,
                      const int64_t* numels) {
    SISIC_REQUIRE(r && names && host_ptrs && numels, "resnet_load: null argument");
    std::vector<int> slot;                    // a refused state dict leaves the handle as it was: nothing below has run
    SISIC_TRY(r->dir.match("resnet_load", n, names, host_ptrs, numels, &slot));
    SISIC_HIP(hipSetDevice(r->ctx->device));
    r->host.assign(r->dir.size(), {});
    for (int i = 0; i < n; ++i) r->host[slot[i]].assign(host_ptrs[i], host_ptrs[i] + numels[i]);
    (void)hipDeviceSynchronize();
    train_free(r);                            // a reload ends training: the arenas described the previous weights
    r->ws_gen = next_workspace_generation();  // every weight buffer moves
    for (auto p : r->owned) (void)hipFree(p);
    r->owned.clear();
    r->loaded = false;
    // which buffers a convolution has depends on its geometry alone: every pointer below is either set again or stays NULL
    SISIC_TRY(fold_alloc(r, r->stem));
    for (auto& b : r->blocks) {
        SISIC_TRY(fold_alloc(r, b.conv1));
        SISIC_TRY(fold_alloc(r, b.conv2));
        SISIC_TRY(fold_alloc(r, b.down));
    }
    SISIC_TRY(dev_alloc(r, r->host[r->fc_w].size(), &r->d_fc_w));
    SISIC_TRY(dev_alloc(r, r->host[r->fc_b].size(), &r->d_fc_b));
    SISIC_TRY(derive_from_host(r, nullptr));
    SISIC_HIP(hipDeviceSynchronize());
    r->loaded = true;
    return SISIC_OK;
}

int sisic_resnet_randomize(sisic_resnet* r, uint64_t seed, uint32_t trial, float strength, void* stream) {
    SISIC_REQUIRE(r, "resnet_randomize: null handle");
    if (!r->loaded) {
        set_error("resnet_randomize called before sisic_resnet_load");
        return SISIC_ESTATE;
    }
    if (r->train) {
        set_error("resnet_randomize: the handle is training (sisic_resnet_train_end first)");
        return SISIC_ESTATE;
    }
    SISIC_HIP(hipSetDevice(r->ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    constexpr uint32_t TAG0 = 16u;           // tag 16 + k: tensor k in sisic_resnet_tensor_name order
    auto conv = [&](FoldedConv& c) -> int {
        if (c.k == 0) return SISIC_OK;
        SISIC_TRY(launch_randomize_weight(r->ctx, c.raw, c.raw_t, c.sc, c.cout, c.cin, c.k, seed, trial, TAG0 + (uint32_t)c.w_idx,
                                          strength, s));
        return fold_pack(r, c, s);
    };
    SISIC_TRY(conv(r->stem));
    for (auto& b : r->blocks) {
        SISIC_TRY(conv(b.conv1));
        SISIC_TRY(conv(b.conv2));
        SISIC_TRY(conv(b.down));
    }
    return launch_randomize_weight(r->ctx, r->d_fc_w, nullptr, nullptr, r->num_classes, 512, 1, seed, trial,
                                   TAG0 + (uint32_t)r->fc_w, strength, s);
}

int sisic_resnet_restore(sisic_resnet* r, void* stream) {
    SISIC_REQUIRE(r, "resnet_restore: null handle");
    if (!r->loaded) {
        set_error("resnet_restore called before sisic_resnet_load");
        return SISIC_ESTATE;
    }
    if (r->train) {
        set_error("resnet_restore: the handle is training (sisic_resnet_train_end first)");
        return SISIC_ESTATE;
    }
    SISIC_HIP(hipSetDevice(r->ctx->device));
    hipStream_t s = static_cast<hipStream_t>(stream);
    SISIC_HIP(hipStreamSynchronize(s));      // launches that still read the filters; the uploads below are blocking copies
    return derive_from_host(r, s);
}

int sisic_resnet_forward(sisic_resnet* r, const float* x, float* logits, int B, int H, int W, int preprocess,
                         void* stream) {
    SISIC_REQUIRE(r && x && logits && B > 0 && H > 0 && W > 0, "resnet_forward: bad arguments");
    SISIC_TRY(begin_run(r, "resnet_forward", B, H, W));
    hipStream_t s = static_cast<hipStream_t>(stream);
    PoolScope ws(r->pool, s);
    Trunk t;
    t.preprocess = preprocess != 0;
    t.logits = logits;
    return run_trunk(r, ws, x, B, H, W, t, s);
}

// The forward up to and including the global average pool: the features the evaluation metrics are computed on.
int sisic_resnet_features(sisic_resnet* r, sisic_resnet_features_args* a) {
    SISIC_REQUIRE(r && a && a->x && a->out && a->B > 0 && a->H > 0 && a->W > 0, "resnet_features: bad arguments");
    SISIC_TRY(begin_run(r, "resnet_features", a->B, a->H, a->W));
    hipStream_t s = static_cast<hipStream_t>(a->stream);
    PoolScope ws(r->pool, s);
    Trunk t;
    t.preprocess = a->preprocess != 0;
    t.features = a->out;
    return run_trunk(r, ws, a->x, a->B, a->H, a->W, t, s);
}

// The stem's activation relu(bn1(conv1(pre(x)))) alone: what the 3x3/2 max-pool chooses its arg-maxima from.  Parity tests
// replay these routes in the CPU autograd pass (tests/test_gpu_classifier.py), so that input-gradient parity is a
// max-abs statement instead of a statistical one.
int sisic_resnet_stem(sisic_resnet* r, const float* x, float* c1_out, int B, int H, int W, int preprocess, void* stream) {
    SISIC_REQUIRE(r && x && c1_out && B > 0 && H > 0 && W > 0, "resnet_stem: bad arguments");
    SISIC_TRY(begin_run(r, "resnet_stem", B, H, W));
    hipStream_t s = static_cast<hipStream_t>(stream);
    PoolScope ws(r->pool, s);
    Trunk t;
    t.preprocess = preprocess != 0;
    t.stem_out = c1_out;
    return run_trunk(r, ws, x, B, H, W, t, s);
}

// d score / d x for score = log(softmax(logits)[target] + 1e-8) (XAI.py:443-459), x the classifier's raw input in
// [-1,1] (pre-processing included): the quantity captum's IntegratedGradients and the plain-gradient fallback of
// XAI.py:1039-1109 differentiate.  Forward with the activations kept, then the transposed network (see
// classifier_bwd.hip); every convolution of the backward pass is a sisic_conv2d launch with transposed filters.
int sisic_resnet_input_gradient(sisic_resnet* r, const float* x, int B, int H, int W, int target, float* grad_x,
                                float* logits_out, void* stream) {
    SISIC_REQUIRE(r && x && grad_x && B > 0 && H > 0 && W > 0, "resnet_input_gradient: bad arguments");
    SISIC_REQUIRE(target >= 0 && target < r->num_classes, "resnet_input_gradient: class %d of %d", target, r->num_classes);
    return resnet_input_gradient_walk(r, x, B, H, W, target, nullptr, grad_x, logits_out, static_cast<hipStream_t>(stream));
}

// The same walk with one target per image.  The targets reach the device in a block of the pool, ordered on the stream.
int sisic_resnet_input_gradient_targets(sisic_resnet* r, sisic_resnet_targets_args* a) {
    SISIC_REQUIRE(r && a && a->x && a->targets && a->grad_x && a->B > 0 && a->H > 0 && a->W > 0,
                  "resnet_input_gradient_targets: bad arguments");
    for (int b = 0; b < a->B; ++b)
        SISIC_REQUIRE(a->targets[b] >= 0 && a->targets[b] < r->num_classes,
                      "resnet_input_gradient_targets: target %lld of image %d is outside [0, %d)", (long long)a->targets[b], b,
                      r->num_classes);
    SISIC_TRY(begin_run(r, "resnet_input_gradient_targets", a->B, a->H, a->W));
    hipStream_t s = static_cast<hipStream_t>(a->stream);
    PoolScope ws(r->pool, s);
    float* tab = nullptr;
    SISIC_TRY(ws.get((size_t)a->B, &tab));
    SISIC_TRY(stage_targets(r, a->targets, a->B, reinterpret_cast<int*>(tab), s));
    return resnet_input_gradient_walk(r, a->x, a->B, a->H, a->W, 0, reinterpret_cast<const int*>(tab), a->grad_x, a->logits_out, s);
}

// Grad-CAM on layer4[-1].conv2 for the raw logit of `target` (xai/XAI.py:2945-3035; see gradcam_kernel): the forward
// pass with the last block's conv2 (+BatchNorm) output kept before the residual add, then one small kernel per image.
// cam: dev [B,224,224] in [0,1] (pytorch_grad_cam's double min-max scaling), logits_out: dev [B,n_classes] or NULL.
int sisic_resnet_gradcam(sisic_resnet* r, const float* x, int B, int H, int W, int target, float* cam, float* logits_out,
                         void* stream) {
    SISIC_REQUIRE(r && x && cam && B > 0 && H > 0 && W > 0, "resnet_gradcam: bad arguments");
    SISIC_REQUIRE(target >= 0 && target < r->num_classes, "resnet_gradcam: class %d of %d", target, r->num_classes);
    SISIC_TRY(begin_run(r, "resnet_gradcam", B, H, W));
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int S = 224;
    SISIC_REQUIRE(H <= S && W <= S, "resnet_gradcam: input %dx%d larger than the classifier's %dx%d", H, W, S, S);
    PoolScope ws(r->pool, s);
    Trunk t;
    t.split_last = true;
    SISIC_TRY(run_trunk(r, ws, x, B, H, W, t, s));
    const FoldedConv& c2 = r->blocks.back().conv2;
    if (logits_out)
        SISIC_HIP(hipMemcpyAsync(logits_out, t.logits, (size_t)B * r->num_classes * sizeof(float), hipMemcpyDeviceToDevice, s));
    return launch_gradcam(r->ctx, t.ylast, t.act, r->d_fc_w, c2.bias, cam, B, c2.cout, t.h, t.w, S, target, s);
}

}  // extern "C"

// ================================================================ training with frozen BatchNorm ====================
namespace {

constexpr int TRAIN_MAX_BATCH = 4096;            // fc_head_bwd_kernel keeps two floats per sample in LDS

int require_train(const sisic_resnet* r, const char* who) {
    SISIC_REQUIRE(r, "%s: null handle", who);
    if (!r->loaded) {
        set_error("%s called before sisic_resnet_load", who);
        return SISIC_ESTATE;
    }
    if (!r->train) {
        set_error("%s called without sisic_resnet_train_begin", who);
        return SISIC_ESTATE;
    }
    return SISIC_OK;
}

template <class F>
int for_each_conv(sisic_resnet* r, F&& f) {
    SISIC_TRY(f(r->stem));
    for (auto& b : r->blocks) {
        SISIC_TRY(f(b.conv1));
        SISIC_TRY(f(b.conv2));
        if (b.down.k) SISIC_TRY(f(b.down));
    }
    return SISIC_OK;
}

// The weight gradient of convolution c (not the stem) from its input `in` [B, cin, h, w] and the gradient dy of its output.
// A 1x1 stride-2 convolution reads the even pixels only: gathered into `even` [B, cin, (h+1)/2, (w+1)/2], its gradient is
// the 1x1 stride-1 form.  Pointers may be NULL when only the scratch size is asked for.
WgradArgs wgrad_args(const FoldedConv& c, const float* in, const float* even, int B, int h, int w, const float* dy, float* dw) {
    WgradArgs a;
    a.c0 = c.cin; a.B = B; a.Cout = c.cout; a.dy = dy; a.dw = dw;
    if (c.k == 1 && c.stride == 2) {
        a.in0 = even; a.Hin = (h - 1) / 2 + 1; a.Win = (w - 1) / 2 + 1; a.ksize = 1; a.stride = 1;
    } else {
        a.in0 = in; a.Hin = h; a.Win = w; a.ksize = c.k; a.stride = c.stride;
    }
    return a;
}

// every plane a stride-2 layer reads has even sizes (the zero-insertion form of its transposed convolution, the stem's weight
// gradient): checked before anything is launched
int check_train_geometry(int H, int W, int preprocess, int bn_batch) {
    int h = preprocess ? 224 : H, w = preprocess ? 224 : W;
    SISIC_REQUIRE(!preprocess || (H <= 224 && W <= 224), "resnet_loss_backward: input %dx%d larger than the classifier's 224x224", H, W);
    SISIC_REQUIRE(h >= 8 && w >= 8 && h % 2 == 0 && w % 2 == 0, "resnet_loss_backward: odd feature map: the stem reads %dx%d (even sizes from 8)", h, w);
    h /= 2; w /= 2;                                       // stem
    SISIC_REQUIRE(h % 2 == 0 && w % 2 == 0, "resnet_loss_backward: odd feature map %dx%d before the max-pool", h, w);
    h /= 2; w /= 2;                                       // max-pool
    for (int l = 1; l < 4; ++l) {
        SISIC_REQUIRE(h % 2 == 0 && w % 2 == 0, "resnet_loss_backward: odd feature map %dx%d before layer%d", h, w, l + 1);
        h /= 2; w /= 2;
    }
    // batch statistics: the last plane's BatchNorm needs more than one value per channel
    SISIC_REQUIRE(bn_batch == 0 || (int64_t)bn_batch * h * w >= 2, "resnet_loss_backward: batch %d at a last plane of %dx%d: BatchNorm "
                  "with batch statistics expects more than 1 value per channel", bn_batch, h, w);
    return SISIC_OK;
}

GradStats* stats_record(ResnetTrain* tr) { return static_cast<GradStats*>(tr->stats); }
float* loss_slot(ResnetTrain* tr) { return reinterpret_cast<float*>(static_cast<char*>(tr->stats) + 12); }
void* stats_scratch(ResnetTrain* tr) { return static_cast<char*>(tr->stats) + 16; }

// ================================================================ batch-statistics BatchNorm ========================
// every form of the UNFOLDED weights from the parameter arena: what the training forward and the walk read
int rebuild_plain_forms(sisic_resnet* r, hipStream_t s) {
    ResnetTrain* tr = r->train;
    SISIC_TRY(launch_conv_pack(r->ctx, param_of(tr, r->stem.w_idx), r->stem.cout, r->stem.cin, r->stem.k, r->stem.u.packed, s));
    for (int p = 0; p < 3; ++p)
        SISIC_TRY(launch_pack_batch(r->ctx, static_cast<const PackJob*>(tr->plain_dev[p]), tr->plain_jobs[p], tr->plain_blocks[p], s));
    return SISIC_OK;
}

// The folded inference forms from (w, gamma, beta, running_mean, running_var) as they stand on the device: the scale and the
// bias in double (launch_bn_fold: fold()'s arithmetic), then the refold and the batched repack of the frozen mode's step.
int refresh_inference_forms(sisic_resnet* r, hipStream_t s) {
    ResnetTrain* tr = r->train;
    SISIC_TRY(for_each_conv(r, [&](FoldedConv& c) {
        SISIC_TRY(launch_bn_fold(r->ctx, param_of(tr, c.bn_w), param_of(tr, c.bn_b), stat_of(tr, c.bn_m), stat_of(tr, c.bn_v), BN_EPS, c.sc,
                                 c.bias, c.cout, s));
        return launch_refold(r->ctx, param_of(tr, c.w_idx), c.sc, c.raw, c.raw_t, c.cout, c.cin, c.k, s);
    }));
    SISIC_TRY(fold_pack(r, r->stem, s));
    for (int p = 0; p < 2; ++p)
        SISIC_TRY(launch_pack_batch(r->ctx, static_cast<const PackJob*>(tr->repack_dev[p]), tr->repack_jobs[p], tr->repack_blocks[p], s));
    SISIC_HIP(hipMemcpyAsync(r->d_fc_w, param_of(tr, r->fc_w), (size_t)r->dir.numels[r->fc_w] * sizeof(float), hipMemcpyDeviceToDevice, s));
    SISIC_HIP(hipMemcpyAsync(r->d_fc_b, param_of(tr, r->fc_b), (size_t)r->dir.numels[r->fc_b] * sizeof(float), hipMemcpyDeviceToDevice, s));
    tr->stats_moved = false;
    return SISIC_OK;
}

// the buffer arena of the running statistics, the second set of filter buffers and its job lists, and the first build of the set
// (the caller, train_begin, has filled the parameter arena and synchronises the device afterwards)
int train_begin_plain(sisic_resnet* r) {
    ResnetTrain* tr = r->train;
    for_each_conv(r, [&](FoldedConv& c) {
        for (int idx : {c.bn_m, c.bn_v}) {
            tr->boff[idx] = (int64_t)tr->buf_floats;
            tr->buf_floats += (size_t)round_up((int)r->dir.numels[idx], 4);
        }
        return SISIC_OK;
    });
    {
        void* p = nullptr;
        SISIC_HIP(hipMalloc(&p, tr->buf_floats * sizeof(float)));
        tr->buf = static_cast<float*>(p);
        SISIC_TRY(poison_fresh(p, tr->buf_floats * sizeof(float)));
        SISIC_HIP(hipMemset(p, 0, tr->buf_floats * sizeof(float)));
    }
    for (int i = 0; i < r->dir.size(); ++i)
        if (tr->boff[i] >= 0)
            SISIC_HIP(hipMemcpy(tr->buf + tr->boff[i], r->host[i].data(), r->host[i].size() * sizeof(float), hipMemcpyHostToDevice));
    auto alloc = [&](size_t floats, float** out) {
        void* p = nullptr;
        SISIC_HIP(hipMalloc(&p, std::max<size_t>(floats, 4) * sizeof(float)));
        tr->plain_owned.push_back(static_cast<float*>(p));
        SISIC_TRY(poison_fresh(p, std::max<size_t>(floats, 4) * sizeof(float)));
        *out = static_cast<float*>(p);
        return SISIC_OK;
    };
    std::vector<PackJob> ph[3];
    SISIC_TRY(alloc((size_t)sisic_conv_packed_numel(r->stem.cout, r->stem.cin, r->stem.k), &r->stem.u.packed));
    auto plan = [&](FoldedConv& c) {
        const float* w = param_of(tr, c.w_idx);
        SISIC_TRY(alloc((size_t)c.cout * c.cin * c.k * c.k, &c.u.raw_t));
        SISIC_TRY(alloc((size_t)sisic_conv_packed_numel(c.cout, c.cin, c.k), &c.u.packed));
        SISIC_TRY(alloc((size_t)sisic_conv_packed_numel(c.cin, c.cout, c.k), &c.u.packed_t));
        ph[0].push_back(pack_job_flip(w, c.cout, c.cin, c.k * c.k, c.u.raw_t));
        ph[0].push_back(pack_job_conv(w, c.cout, c.cin, c.k, c.u.packed));
        ph[1].push_back(pack_job_conv(c.u.raw_t, c.cin, c.cout, c.k, c.u.packed_t));
        if (c.wino) {
            SISIC_TRY(alloc((size_t)winograd_packed_numel(c.cout, c.cin), &c.u.wino));
            SISIC_TRY(alloc((size_t)winograd_packed_numel(c.cin, c.cout), &c.u.wino_t));
            ph[0].push_back(pack_job_wino_first(w, c.cout, c.cin, c.u.wino));
            ph[1].push_back(pack_job_wino_wide(c.cout, c.cin, c.u.wino));
            ph[1].push_back(pack_job_wino_bf3(c.cout, c.cin, c.u.wino));
            ph[1].push_back(pack_job_wino_first(c.u.raw_t, c.cin, c.cout, c.u.wino_t));
            ph[2].push_back(pack_job_wino_wide(c.cin, c.cout, c.u.wino_t));
            ph[2].push_back(pack_job_wino_bf3(c.cin, c.cout, c.u.wino_t));
        }
        return SISIC_OK;
    };
    for (Block& b : r->blocks) {
        SISIC_TRY(plan(b.conv1));
        SISIC_TRY(plan(b.conv2));
        if (b.down.k) SISIC_TRY(plan(b.down));
    }
    for (int p = 0; p < 3; ++p) SISIC_TRY(upload_pack_table(ph[p], &tr->plain_dev[p], &tr->plain_jobs[p], &tr->plain_blocks[p]));
    return rebuild_plain_forms(r, nullptr);
}

// ================================================================ the backward walk ==================================
// the labels (and class weights) a loss_backward call staged on the host, on the device: one block, ints first
int stage_labels(PoolScope& ws, ResnetTrain* tr, int B, int n, bool class_weights, float** lab, hipStream_t s) {
    SISIC_TRY(ws.get((size_t)B + n, lab));
    SISIC_HIP(hipMemcpyAsync(*lab, tr->labels_host.data(), (size_t)B * sizeof(int), hipMemcpyHostToDevice, s));
    if (class_weights) SISIC_HIP(hipMemcpyAsync(*lab + B, tr->cw_host.data(), (size_t)n * sizeof(float), hipMemcpyHostToDevice, s));
    return SISIC_OK;
}

// the weight gradient of c (wgrad_args) into the gradient arena
int wgrad(sisic_resnet* r, ResnetTrain* tr, const FoldedConv& c, const float* in, const float* even, int B, int h, int w, const float* dy,
          hipStream_t s) {
    const WgradArgs wa = wgrad_args(c, in, even, B, h, w, dy, grad_of(tr, c.w_idx));
    return launch_conv_wgrad(r->ctx, wa, tr->part, tr->part_floats, s);
}

// dy (a new block) = BatchNorm backward of g (masked by act > 0 first when act is given); dgamma and dbeta into the gradient arena;
// y and the moments go back to the pool
int bn_bwd(sisic_resnet* r, PoolScope& ws, ResnetTrain* tr, const FoldedConv& c, const BnKept& k, const float* g, const float* act, int B,
           float** dy, hipStream_t s) {
    SISIC_TRY(ws.get((size_t)B * k.C * k.HW, dy));
    SISIC_TRY(launch_bn_bwd(r->ctx, g, k.y, act, k.st, k.st + k.C, param_of(tr, c.bn_w), *dy, grad_of(tr, c.bn_w), grad_of(tr, c.bn_b), B,
                            k.C, k.HW, s));
    ws.put(k.y);
    ws.put(k.st);
    return SISIC_OK;
}

// What the walk is asked for.  train == nullptr: the input gradient of the score of `target` (or of targets_dev[b]) into grad_x,
// through the stem and the pre-processing; nothing on this path synchronises, waits on the host or allocates on a warm pool (a
// captured sampling step runs it).  train: the cross-entropy loss against the staged labels and the weight gradients, down to
// the stem's; with the trunk's `bn` option a BatchNorm backward stands in front of every weight gradient and transposed
// convolution and the unfolded filters are read, without it the gradients of the folded filters are unfolded at the end.
struct Walk {
    int target = 0;
    const int* targets_dev = nullptr;
    float* grad_x = nullptr;
    ResnetTrain* train = nullptr;
    float* lab = nullptr;            // stage_labels' block
    bool class_weights = false;
    float* loss_out = nullptr;       // host
};

// The transposed network behind run_trunk(t) with its activations kept: the head, the eight blocks last to first (at each the
// gradient g at the block's output, already ReLU-masked, becomes the one at its input), the max-pool, then the mode's tail.  A
// weight gradient is issued from the tensors the walk holds anyway -- the gradient at conv2's and at downsample's output is g,
// the one at conv1's output is tmp after the mask of t1 (with batch statistics: their BatchNorm backwards dy2, dyd and dy1, the
// last of which applies the mask from the kept t1), the inputs are the kept activations.  Every block of the pool the forward
// kept goes back here.  x: the trunk's input [B, 3, H, W].
int backward_walk(sisic_resnet* r, PoolScope& ws, const Trunk& t, const float* x, int B, int H, int W, const Walk& o, float* logits_out,
                  hipStream_t s) {
    ResnetTrain* tr = o.train;
    const bool bn = t.bn != nullptr;
    const int n = r->num_classes, C = r->blocks.back().conv2.cout, c1h = t.c1h, c1w = t.c1w;
    const std::vector<Trunk::Saved>& saved = t.saved;
    if (logits_out) SISIC_HIP(hipMemcpyAsync(logits_out, t.logits, (size_t)B * n * sizeof(float), hipMemcpyDeviceToDevice, s));

    // ---- head
    float* g = nullptr;
    if (!tr) {
        SISIC_TRY(ws.get((size_t)B * C * t.h * t.w, &g));
        if (o.targets_dev)
            SISIC_TRY(launch_score_head_bwd_targets(r->ctx, t.logits, r->d_fc_w, t.act, g, B, C, t.h * t.w, n, o.targets_dev, s));
        else
            SISIC_TRY(launch_score_head_bwd(r->ctx, t.logits, r->d_fc_w, t.act, g, B, C, t.h * t.w, n, o.target, s));
        ws.put(t.logits);
    } else {
        float* dlogits = nullptr;
        SISIC_TRY(ws.get((size_t)B * n, &dlogits));
        SISIC_TRY(launch_ce_head(r->ctx, t.logits, reinterpret_cast<const int*>(o.lab), o.class_weights ? o.lab + B : nullptr, B, n,
                                 loss_slot(tr), dlogits, s));
        SISIC_TRY(ws.get((size_t)B * C * t.h * t.w, &g));
        SISIC_TRY(launch_fc_head_bwd(r->ctx, dlogits, bn ? param_of(tr, r->fc_w) : r->d_fc_w, t.act, g, grad_of(tr, r->fc_w),
                                     grad_of(tr, r->fc_b), B, C, t.h * t.w, n, s));
        ws.put(dlogits);
        ws.put(t.logits);
        ws.put(o.lab);
    }
    // ---- the blocks, last to first
    for (int k = (int)r->blocks.size() - 1; k >= 0; --k) {
        const Block& b = r->blocks[k];
        const Trunk::Saved& sv = saved[k];
        const float* in_act = k > 0 ? saved[k - 1].out : t.m;          // the block's input [B, conv1.cin, sv.h, sv.w]
        const ConvForms f1 = forms_of(b.conv1, bn), f2 = forms_of(b.conv2, bn), fd = forms_of(b.down, bn);
        float* dy2 = g;                                   // the gradient at conv2's output
        if (bn) SISIC_TRY(bn_bwd(r, ws, tr, b.conv2, sv.k2, g, nullptr, B, &dy2, s));
        if (tr) SISIC_TRY(wgrad(r, tr, b.conv2, sv.t1, nullptr, B, sv.bh, sv.bw, dy2, s));
        const size_t n_mid = (size_t)B * b.conv2.cout * sv.bh * sv.bw;
        float* tmp = nullptr;                             // conv2^T dy2 = the gradient at t1, before its ReLU mask
        SISIC_TRY(ws.get(n_mid, &tmp));
        SISIC_TRY(conv_t(r, b.conv2, f2, dy2, B, sv.bh, sv.bw, nullptr, tmp, s));
        float* dy1 = tmp;                                 // the gradient at conv1's output, masked
        if (bn) {
            ws.put(dy2);
            SISIC_TRY(bn_bwd(r, ws, tr, b.conv1, sv.k1, tmp, sv.t1, B, &dy1, s));
            ws.put(tmp);
        } else {
            SISIC_TRY(launch_relu_bwd(r->ctx, tmp, sv.t1, tmp, (int64_t)n_mid, s));
        }
        if (tr) SISIC_TRY(wgrad(r, tr, b.conv1, in_act, nullptr, B, sv.h, sv.w, dy1, s));
        const size_t n_in = (size_t)B * b.conv1.cin * sv.h * sv.w;
        float* da = nullptr;
        SISIC_TRY(ws.get(n_in, &da));
        if (!b.down.k) {
            SISIC_TRY(conv_t(r, b.conv1, f1, dy1, B, sv.bh, sv.bw, g, da, s));        // + identity path
        } else {
            SISIC_TRY(conv_t(r, b.conv1, f1, dy1, B, sv.bh, sv.bw, nullptr, da, s));  // stride 2: zero-insertion input
            float* dyd = g;                               // the gradient at downsample's output
            if (bn) SISIC_TRY(bn_bwd(r, ws, tr, b.down, sv.kd, g, nullptr, B, &dyd, s));
            float* small = nullptr;
            SISIC_TRY(ws.get((size_t)B * b.down.cin * sv.bh * sv.bw, &small));
            if (tr) {                                     // first the even pixels of the input (ResNet18's downsamples are stride 2) ...
                SISIC_TRY(launch_gather_even(r->ctx, in_act, small, B * b.down.cin, sv.h, sv.w, s));
                SISIC_TRY(wgrad(r, tr, b.down, nullptr, small, B, sv.h, sv.w, dyd, s));
            }
            SISIC_TRY(conv_t(r, b.down, fd, dyd, B, sv.bh, sv.bw, nullptr, small, s));  // ... then the 1x1 at the low resolution
            SISIC_TRY(launch_scatter_add_even(r->ctx, da, small, B * b.down.cin, sv.h, sv.w, s));
            ws.put(small);
            if (bn) ws.put(dyd);
        }
        ws.put(dy1);
        ws.put(g);
        ws.put(sv.t1);
        ws.put(sv.out);
        if (k > 0) SISIC_TRY(launch_relu_bwd(r->ctx, da, saved[k - 1].out, da, (int64_t)n_in, s));      // ReLU of the previous block's output
        g = da;
    }
    // ---- g = the gradient at the max-pool output
    float* dc1 = nullptr;
    SISIC_TRY(ws.get((size_t)B * 64 * c1h * c1w, &dc1));
    SISIC_TRY(launch_maxpool_bwd(r->ctx, g, t.c1, dc1, B * 64, c1h, c1w, s));       // includes the stem's ReLU mask
    ws.put(g);
    ws.put(t.m);
    ws.put(t.c1);
    const int sh = t.preprocess ? 224 : H, sw = t.preprocess ? 224 : W;             // the stem's input plane
    if (!tr) {
        float* dp = nullptr;
        SISIC_TRY(ws.get((size_t)B * 3 * sh * sw, &dp));
        SISIC_TRY(launch_stem_bwd(r->ctx, dc1, r->stem.raw, dp, B, 64, c1h, c1w, sh, sw, s));
        ws.put(dc1);
        SISIC_TRY(launch_preprocess_bwd(r->ctx, dp, x, o.grad_x, B, H, W, sh, sw, s));
        ws.put(dp);
        return SISIC_OK;
    }
    // training stops at the stem's weight gradient: nothing below it is trainable
    float* dys = dc1;                                     // the gradient at the stem convolution's output
    if (bn) {
        SISIC_TRY(bn_bwd(r, ws, tr, r->stem, t.stem_k, dc1, nullptr, B, &dys, s));
        ws.put(dc1);
    }
    SISIC_TRY(launch_stem_wgrad(r->ctx, t.pre ? t.pre : x, dys, grad_of(tr, r->stem.w_idx), B, sh, sw, tr->part, tr->part_floats, s));
    ws.put(dys);
    if (t.pre) ws.put(t.pre);
    if (!bn)                                              // the chain differentiated the folded filters
        SISIC_TRY(for_each_conv(r, [&](FoldedConv& c) { return launch_unfold_grad(r->ctx, grad_of(tr, c.w_idx), c.sc, c.cout, c.cin, c.k, s); }));
    SISIC_HIP(hipMemcpyAsync(o.loss_out, loss_slot(tr), sizeof(float), hipMemcpyDeviceToHost, s));
    SISIC_HIP(hipStreamSynchronize(s));
    return SISIC_OK;
}

int train_begin(sisic_resnet* r, int bn_mode, double momentum) {
    SISIC_REQUIRE(r, "resnet_train_begin: null handle");
    if (!r->loaded) {
        set_error("resnet_train_begin called before sisic_resnet_load");
        return SISIC_ESTATE;
    }
    if (r->train) {
        set_error("resnet_train_begin: the handle is training already");
        return SISIC_ESTATE;
    }
    SISIC_HIP(hipSetDevice(r->ctx->device));
    SISIC_HIP(hipDeviceSynchronize());
    auto* tr = new ResnetTrain();
    r->train = tr;                               // (freed by train_end, a reload or destroy, also after an error below)
    r->ws_gen = next_workspace_generation();
    tr->bn_mode = bn_mode;
    tr->momentum = momentum;
    tr->off.assign(r->dir.size(), -1);
    tr->boff.assign(r->dir.size(), -1);
    auto place = [&](int idx) {
        tr->off[idx] = (int64_t)tr->floats;
        tr->floats += (size_t)round_up((int)r->dir.numels[idx], 4);
    };
    std::vector<char> trainable(r->dir.size(), 0);
    for_each_conv(r, [&](FoldedConv& c) {
        trainable[c.w_idx] = 1;
        if (bn_mode == 1) trainable[c.bn_w] = trainable[c.bn_b] = 1;
        return SISIC_OK;
    });
    trainable[r->fc_w] = trainable[r->fc_b] = 1;
    for (int i = 0; i < r->dir.size(); ++i)
        if (trainable[i]) place(i);
    // the partial slabs: the most any layer asks for at any shape (its K-split is capped by the layer's tile count)
    tr->part_floats = stem_wgrad_scratch_floats();
    {
        int h = 56;                              // layer1's plane at the classifier's 224x224; larger inputs reach the same caps
        for (const Block& b : r->blocks) {
            const int bh = out_dim(h, 3, b.conv1.stride);
            tr->part_floats = std::max(tr->part_floats, conv_wgrad_scratch_floats(wgrad_args(b.conv1, nullptr, nullptr, TRAIN_MAX_BATCH, h, h, nullptr, nullptr)));
            tr->part_floats = std::max(tr->part_floats, conv_wgrad_scratch_floats(wgrad_args(b.conv2, nullptr, nullptr, TRAIN_MAX_BATCH, bh, bh, nullptr, nullptr)));
            if (b.down.k)
                tr->part_floats = std::max(tr->part_floats, conv_wgrad_scratch_floats(wgrad_args(b.down, nullptr, nullptr, TRAIN_MAX_BATCH, h, h, nullptr, nullptr)));
            h = bh;
        }
    }
    const size_t bytes = tr->floats * sizeof(float);
    for (float** q : {&tr->param, &tr->grad, &tr->adam_m, &tr->adam_v}) {
        void* p = nullptr;
        SISIC_HIP(hipMalloc(&p, bytes));
        *q = static_cast<float*>(p);
        SISIC_TRY(poison_fresh(p, bytes));
        SISIC_HIP(hipMemset(p, 0, bytes));
    }
    {
        void* p = nullptr;
        SISIC_HIP(hipMalloc(&p, tr->part_floats * sizeof(float)));
        tr->part = static_cast<float*>(p);
        SISIC_TRY(poison_fresh(p, tr->part_floats * sizeof(float)));
        const size_t sb = 16 + grad_stats_scratch_bytes();
        SISIC_HIP(hipMalloc(&tr->stats, sb));
        SISIC_TRY(poison_fresh(tr->stats, sb));
    }
    for (int i = 0; i < r->dir.size(); ++i)
        if (tr->off[i] >= 0)
            SISIC_HIP(hipMemcpy(tr->param + tr->off[i], r->host[i].data(), r->host[i].size() * sizeof(float), hipMemcpyHostToDevice));
    {
        std::vector<PackJob> ph[2];
        auto plan = [&](const FoldedConv& c) {
            ph[0].push_back(pack_job_conv(c.raw, c.cout, c.cin, c.k, c.packed));
            ph[0].push_back(pack_job_conv(c.raw_t, c.cin, c.cout, c.k, c.packed_t));
            if (c.wino) {
                ph[0].push_back(pack_job_wino_first(c.raw, c.cout, c.cin, c.wino));
                ph[1].push_back(pack_job_wino_wide(c.cout, c.cin, c.wino));
                ph[1].push_back(pack_job_wino_bf3(c.cout, c.cin, c.wino));
                ph[0].push_back(pack_job_wino_first(c.raw_t, c.cin, c.cout, c.wino_t));
                ph[1].push_back(pack_job_wino_wide(c.cin, c.cout, c.wino_t));
                ph[1].push_back(pack_job_wino_bf3(c.cin, c.cout, c.wino_t));
            }
        };
        for (const Block& b : r->blocks) {
            plan(b.conv1);
            plan(b.conv2);
            if (b.down.k) plan(b.down);
        }
        for (int p = 0; p < 2; ++p) SISIC_TRY(upload_pack_table(ph[p], &tr->repack_dev[p], &tr->repack_jobs[p], &tr->repack_blocks[p]));
    }
    if (bn_mode == 1) SISIC_TRY(train_begin_plain(r));
    SISIC_HIP(hipDeviceSynchronize());
    return SISIC_OK;
}

}  // namespace

sisic_ctx* sisic::resnet_ctx(const sisic_resnet* r) { return r->ctx; }
bool sisic::resnet_loaded(const sisic_resnet* r) { return r->loaded; }
int sisic::resnet_num_classes(const sisic_resnet* r) { return r->num_classes; }
uint64_t sisic::resnet_workspace_generation(const sisic_resnet* r) { return r->ws_gen; }

// The input gradient (sisic_resnet_input_gradient[_targets], and each classifier-guided step of sisic_sample_frames_clf, there
// under stream capture): the forward with the activations kept, then the walk in its input-gradient form.
int sisic::resnet_input_gradient_walk(sisic_resnet* r, const float* x, int B, int H, int W, int target, const int* targets_dev,
                                      float* grad_x, float* logits_out, hipStream_t s) {
    SISIC_TRY(begin_run(r, "resnet_input_gradient", B, H, W));
    PoolScope ws(r->pool, s);
    SISIC_REQUIRE(H <= 224 && W <= 224, "resnet_input_gradient: input %dx%d larger than the classifier's %dx%d", H, W, 224, 224);
    Trunk t;
    t.keep = true;
    SISIC_TRY(run_trunk(r, ws, x, B, H, W, t, s));
    Walk o;
    o.target = target;
    o.targets_dev = targets_dev;
    o.grad_x = grad_x;
    return backward_walk(r, ws, t, x, B, H, W, o, logits_out, s);
}

extern "C" {

int sisic_resnet_train_begin(sisic_resnet* r) { return train_begin(r, 0, 0.0); }

int sisic_resnet_train_begin_bn(sisic_resnet* r, const sisic_resnet_bn_config* config) {
    SISIC_REQUIRE(r && config, "resnet_train_begin_bn: null argument");
    SISIC_REQUIRE(config->mode == 0 || config->mode == 1, "resnet_train_begin_bn: mode %d (0 frozen, 1 batch statistics)", config->mode);
    if (config->mode == 0) return train_begin(r, 0, 0.0);
    SISIC_REQUIRE(config->momentum > 0.0 && config->momentum <= 1.0, "resnet_train_begin_bn: momentum %g is outside (0, 1]", config->momentum);
    return train_begin(r, 1, config->momentum);
}

int sisic_resnet_train_bn_mode(const sisic_resnet* r) { return (r && r->train) ? r->train->bn_mode : -1; }

// The device already holds what sisic_resnet_load of the trained state dict would leave (optimizer_step derives every form with
// the load path's arithmetic); the host copies that sisic_resnet_restore folds from follow here.
int sisic_resnet_train_end(sisic_resnet* r) {
    SISIC_TRY(require_train(r, "resnet_train_end"));
    ResnetTrain* tr = r->train;
    SISIC_HIP(hipSetDevice(r->ctx->device));
    if (tr->bn_mode == 1 && tr->stats_moved) SISIC_TRY(refresh_inference_forms(r, nullptr));
    SISIC_HIP(hipDeviceSynchronize());
    for (int i = 0; i < r->dir.size(); ++i) {
        if (tr->off[i] >= 0)
            SISIC_HIP(hipMemcpy(r->host[i].data(), tr->param + tr->off[i], r->host[i].size() * sizeof(float), hipMemcpyDeviceToHost));
        if (tr->boff[i] >= 0)
            SISIC_HIP(hipMemcpy(r->host[i].data(), tr->buf + tr->boff[i], r->host[i].size() * sizeof(float), hipMemcpyDeviceToHost));
    }
    train_free(r);
    r->ws_gen = next_workspace_generation();
    return SISIC_OK;
}

int64_t sisic_resnet_train_steps(const sisic_resnet* r) { return (r && r->train) ? r->train->step : 0; }

int sisic_resnet_zero_grad(sisic_resnet* r) {
    SISIC_TRY(require_train(r, "resnet_zero_grad"));
    SISIC_HIP(hipSetDevice(r->ctx->device));
    SISIC_HIP(hipDeviceSynchronize());
    SISIC_HIP(hipMemset(r->train->grad, 0, r->train->floats * sizeof(float)));
    SISIC_HIP(hipDeviceSynchronize());
    return SISIC_OK;
}

// sisic_resnet_read / _write: tensor `index` of arena `what` to the host, or (write) from it; synchronises unless the host has it
static int resnet_transfer(sisic_resnet* r, const char* who, bool write, int what, int index, float* host, int64_t numel) {
    SISIC_REQUIRE(r, "%s: bad arguments", who);
    SISIC_TRY(r->dir.check_access(who, index, numel, host));
    SISIC_REQUIRE(!write || what != 0, "%s: parameters are set by sisic_resnet_load (their folded and packed forms must follow); "
                                       "what = 1 gradient, 2 Adam m, 3 Adam v", who);
    SISIC_REQUIRE(what >= 0 && what <= 3, "%s: what = %d (%s1 gradient, 2 Adam m, 3 Adam v)", who, what, write ? "" : "0 parameter, ");
    if (!write && !r->loaded) {
        set_error("resnet_read called before sisic_resnet_load");
        return SISIC_ESTATE;
    }
    ResnetTrain* tr = r->train;
    float* dev = nullptr;
    if (what == 0 && tr && tr->boff[index] >= 0) {        // a running statistic of batch-statistics training: its current value
        dev = tr->buf + tr->boff[index];
    } else if (what == 0 && (!tr || tr->off[index] < 0)) {   // frozen, or not training: the loaded value
        std::memcpy(host, r->host[index].data(), (size_t)numel * sizeof(float));
        return SISIC_OK;
    } else {
        SISIC_TRY(require_train(r, who));
        SISIC_REQUIRE(tr->boff[index] < 0, "%s: '%s' is a running statistic: it has no gradient or moment", who, r->dir.name(index));
        SISIC_REQUIRE(tr->off[index] >= 0, "%s: '%s' is frozen (BatchNorm): it has no gradient or moment", who, r->dir.name(index));
        dev = (what == 0 ? tr->param : what == 1 ? tr->grad : what == 2 ? tr->adam_m : tr->adam_v) + tr->off[index];
    }
    SISIC_HIP(hipSetDevice(r->ctx->device));
    SISIC_HIP(hipDeviceSynchronize());
    SISIC_HIP(hipMemcpy(write ? dev : host, write ? host : dev, (size_t)numel * sizeof(float), write ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost));
    return SISIC_OK;
}

int sisic_resnet_read(sisic_resnet* r, int what, int index, float* out, int64_t numel) { return resnet_transfer(r, "resnet_read", false, what, index, out, numel); }

int sisic_resnet_write(sisic_resnet* r, int what, int index, const float* in, int64_t numel) {
    return resnet_transfer(r, "resnet_write", true, what, index, const_cast<float*>(in), numel);
}

// loss = cross_entropy(resnet18(x), labels, weight) and its gradient with respect to the trainable tensors: the 22 with BatchNorm
// frozen, the 62 with batch statistics (which also move the running statistics).  The checks, run_trunk with everything kept,
// then backward_walk seeded by d loss / d logits.
int sisic_resnet_loss_backward(sisic_resnet* r, sisic_resnet_train_args* a) {
    SISIC_TRY(require_train(r, "resnet_loss_backward"));
    SISIC_REQUIRE(a && a->x && a->labels && a->B > 0 && a->H > 0 && a->W > 0, "resnet_loss_backward: bad arguments");
    const int B = a->B, H = a->H, W = a->W, n = r->num_classes;
    SISIC_REQUIRE(B <= TRAIN_MAX_BATCH, "resnet_loss_backward: batch %d (at most %d)", B, TRAIN_MAX_BATCH);
    ResnetTrain* tr = r->train;
    tr->labels_host.resize(B);
    double picked = 0.0;
    for (int b = 0; b < B; ++b) {
        SISIC_REQUIRE(a->labels[b] >= 0 && a->labels[b] < n, "resnet_loss_backward: label %lld of sample %d is outside [0, %d)",
                      (long long)a->labels[b], b, n);
        tr->labels_host[b] = (int)a->labels[b];
        picked += a->class_weights ? (double)a->class_weights[a->labels[b]] : 1.0;
    }
    if (a->class_weights) {
        for (int k = 0; k < n; ++k)
            SISIC_REQUIRE(std::isfinite(a->class_weights[k]) && a->class_weights[k] >= 0.0f, "resnet_loss_backward: class weight %d is %g", k, a->class_weights[k]);
        SISIC_REQUIRE(picked > 0.0, "resnet_loss_backward: the weights of the batch's classes sum to zero");
        tr->cw_host.assign(a->class_weights, a->class_weights + n);
    }
    SISIC_TRY(check_train_geometry(H, W, a->preprocess, tr->bn_mode == 1 ? B : 0));
    SISIC_TRY(begin_run(r, "resnet_loss_backward", B, H, W));
    hipStream_t s = static_cast<hipStream_t>(a->stream);
    PoolScope ws(r->pool, s);
    Walk o;
    o.train = tr;
    o.class_weights = a->class_weights != nullptr;
    o.loss_out = &a->loss;
    SISIC_TRY(stage_labels(ws, tr, B, n, o.class_weights, &o.lab, s));
    Trunk t;
    t.preprocess = a->preprocess != 0;
    t.keep = true;
    t.keep_pre = true;
    t.who = "resnet_loss_backward";
    if (tr->bn_mode == 1) t.bn = tr;
    SISIC_TRY(run_trunk(r, ws, a->x, B, H, W, t, s));
    return backward_walk(r, ws, t, a->x, B, H, W, o, a->logits_out, s);
}

// clip_grad_norm_ (optional) + torch.optim.Adam on the arenas, then every derived form of the new weights.
int sisic_resnet_optimizer_step(sisic_resnet* r, sisic_resnet_train_args* a) {
    SISIC_TRY(require_train(r, "resnet_optimizer_step"));
    SISIC_REQUIRE(a, "resnet_optimizer_step: null arguments");
    SISIC_REQUIRE(a->lr >= 0.0 && a->beta1 >= 0.0 && a->beta1 < 1.0 && a->beta2 >= 0.0 && a->beta2 < 1.0 && a->eps >= 0.0,
                  "resnet_optimizer_step: lr %g betas (%g, %g) eps %g", a->lr, a->beta1, a->beta2, a->eps);
    ResnetTrain* tr = r->train;
    SISIC_HIP(hipSetDevice(r->ctx->device));
    hipStream_t s = static_cast<hipStream_t>(a->stream);
    AdamStepArgs o;
    o.p = tr->param; o.g = tr->grad; o.m = tr->adam_m; o.v = tr->adam_v; o.n = tr->floats;
    o.lr = a->lr; o.beta1 = a->beta1; o.beta2 = a->beta2; o.eps = a->eps; o.max_norm = a->max_grad_norm;
    o.step = &tr->step; o.stats = stats_record(tr); o.scratch = stats_scratch(tr);
    o.want_stats = o.skip_on_inf = true;
    AdamStepResult res;
    SISIC_TRY(adam_step(r->ctx, o, &res, s));
    a->grad_norm = res.norm;
    a->found_inf = res.found_inf;
    if (tr->bn_mode == 1) {
        // batch statistics: the running statistics moved in loss_backward whether or not the update is skipped, so the inference
        // forms are derived again on every call
        if (!res.skipped) SISIC_TRY(rebuild_plain_forms(r, s));
        return refresh_inference_forms(r, s);
    }
    if (res.skipped) return SISIC_OK;                    // no update: parameters, moments and the step counter stay
    SISIC_TRY(for_each_conv(r, [&](FoldedConv& c) {
        return launch_refold(r->ctx, tr->param + tr->off[c.w_idx], c.sc, c.raw, c.raw_t, c.cout, c.cin, c.k, s);
    }));
    SISIC_TRY(fold_pack(r, r->stem, s));                 // the 7x7 filter: one form, the load path's launch
    for (int p = 0; p < 2; ++p)
        SISIC_TRY(launch_pack_batch(r->ctx, static_cast<const PackJob*>(tr->repack_dev[p]), tr->repack_jobs[p], tr->repack_blocks[p], s));
    SISIC_HIP(hipMemcpyAsync(r->d_fc_w, tr->param + tr->off[r->fc_w], (size_t)r->dir.numels[r->fc_w] * sizeof(float), hipMemcpyDeviceToDevice, s));
    SISIC_HIP(hipMemcpyAsync(r->d_fc_b, tr->param + tr->off[r->fc_b], (size_t)r->dir.numels[r->fc_b] * sizeof(float), hipMemcpyDeviceToDevice, s));
    return SISIC_OK;
}

int sisic_class_scores(sisic_ctx* ctx, const float* logits, int B, int n_classes, int target, float* prob,
                       float* logscore, void* stream) {
    SISIC_REQUIRE(ctx, "class_scores: null context");
    return launch_class_scores(ctx, logits, B, n_classes, target, prob, logscore, static_cast<hipStream_t>(stream));
}

int sisic_mask_patches(sisic_ctx* ctx, const float* image, const uint8_t* masks, float* out, int S, int C, int H, int W,
                       int patch, void* stream) {
    SISIC_REQUIRE(ctx, "mask_patches: null context");
    return launch_mask_patches(ctx, image, masks, out, S, C, H, W, patch, static_cast<hipStream_t>(stream));
}

}  // extern "C"
