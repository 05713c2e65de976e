// unet.cpp -- the UNet2DModel executor and the reverse-diffusion loop.
//
// Walks the architecture the reference configures at core/generator/model_manager.py:173-194
//  and issues the fused HIP kernels:
//     ResnetBlock2D  = gn_stats -> conv3x3[GN+SiLU prologue, +bias +time-embedding]
//                      -> gn_stats -> conv3x3[GN+SiLU prologue, +bias +shortcut/residual]
//                      (conv1x1 shortcut on the raw, possibly concatenated input when Cin != Cout)
//     Attention      = gn_stats -> conv1x1[GN prologue] (q,k,v in one launch) -> attention core
//                      -> conv1x1[+bias +residual]
//     Downsample2D   = conv3x3 stride 2;   Upsample2D = conv3x3 reading through a nearest-2x map
// torch.cat of the skip connections never materialises: consumers read two source tensors.
// sisic_sample() runs the loop of core/generator/image_generator.py:395-403 without returning
// to the host between steps.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>

#include "conv_plan.h"
#include "gn_finalize.h"
#include "train.h"
#include "unet_internal.h"

using namespace sisic;

namespace {

// ------------------------------------------------------------------ architecture description
void add_conv(sisic_unet* u, ConvW& c, const std::string& name, int cout, int cin, int k) {
    c.cout = cout; c.cin = cin; c.k = k;
    c.w_idx = u->add(name + ".weight", (int64_t)cout * cin * k * k);
    c.b_idx = u->add(name + ".bias", cout);
}
void add_norm(sisic_unet* u, NormW& n, const std::string& name, int c) {
    n.c = c;
    n.w_idx = u->add(name + ".weight", c);
    n.b_idx = u->add(name + ".bias", c);
}
void add_resnet(sisic_unet* u, ResnetW& r, const std::string& name, int cin, int cout) {
    r.cin = cin; r.cout = cout;
    add_norm(u, r.norm1, name + ".norm1", cin);
    add_conv(u, r.conv1, name + ".conv1", cout, cin, 3);
    r.temb_w_idx = u->add(name + ".time_emb_proj.weight", (int64_t)cout * u->hidden);
    r.temb_b_idx = u->add(name + ".time_emb_proj.bias", cout);
    r.temb_off = u->tproj_R;
    u->tproj_R += cout;
    add_norm(u, r.norm2, name + ".norm2", cout);
    add_conv(u, r.conv2, name + ".conv2", cout, cout, 3);
    if (cin != cout) add_conv(u, r.shortcut, name + ".conv_shortcut", cout, cin, 1);
    u->max_c = std::max(u->max_c, std::max(cin, cout));
}
void add_attn(sisic_unet* u, AttnW& a, const std::string& name, int c) {
    a.c = c;
    add_norm(u, a.norm, name + ".group_norm", c);
    a.q_w = u->add(name + ".to_q.weight", (int64_t)c * c); a.q_b = u->add(name + ".to_q.bias", c);
    a.k_w = u->add(name + ".to_k.weight", (int64_t)c * c); a.k_b = u->add(name + ".to_k.bias", c);
    a.v_w = u->add(name + ".to_v.weight", (int64_t)c * c); a.v_b = u->add(name + ".to_v.bias", c);
    add_conv(u, a.out, name + ".to_out.0", c, c, 1);
    u->max_c = std::max(u->max_c, c);
}

int describe(sisic_unet* u) {
    const sisic_unet_config& cfg = u->cfg;
    const int n = cfg.n_blocks;
    const int* boc = cfg.block_out_channels;
    u->hidden = 4 * boc[0];
    add_conv(u, u->conv_in, "conv_in", boc[0], cfg.in_channels, 3);
    u->temb_w1 = u->add("time_embedding.linear_1.weight", (int64_t)u->hidden * boc[0]);
    u->temb_b1 = u->add("time_embedding.linear_1.bias", u->hidden);
    u->temb_w2 = u->add("time_embedding.linear_2.weight", (int64_t)u->hidden * u->hidden);
    u->temb_b2 = u->add("time_embedding.linear_2.bias", u->hidden);
    // UNet2DModel registers its modules as conv_in, time_proj, time_embedding, class_embedding, down_blocks, ...: the
    // nn.Embedding(num_class_embeds, time_embed_dim) of a conditional model has its one tensor here in the state dict
    if (u->n_class > 0) u->class_w = u->add("class_embedding.weight", (int64_t)u->n_class * u->hidden);

    u->down_res.resize(n); u->down_attn.resize(n); u->downsamplers.resize(n);
    int out_ch = boc[0];
    for (int i = 0; i < n; ++i) {
        const int in_ch = out_ch;
        out_ch = boc[i];
        u->down_res[i].resize(cfg.layers_per_block);
        if (cfg.down_attn[i]) u->down_attn[i].resize(cfg.layers_per_block);
        for (int j = 0; j < cfg.layers_per_block; ++j) {
            const std::string base = "down_blocks." + std::to_string(i);
            add_resnet(u, u->down_res[i][j], base + ".resnets." + std::to_string(j), j == 0 ? in_ch : out_ch, out_ch);
            if (cfg.down_attn[i]) add_attn(u, u->down_attn[i][j], base + ".attentions." + std::to_string(j), out_ch);
        }
        if (i != n - 1) {
            add_conv(u, u->downsamplers[i], "down_blocks." + std::to_string(i) + ".downsamplers.0.conv", out_ch, out_ch, 3);
            u->downsamplers[i].strided = true;
        }
    }
    const int mid = boc[n - 1];
    add_resnet(u, u->mid_res[0], "mid_block.resnets.0", mid, mid);
    add_attn(u, u->mid_attn, "mid_block.attentions.0", mid);
    add_resnet(u, u->mid_res[1], "mid_block.resnets.1", mid, mid);

    u->up_res.resize(n); u->up_attn.resize(n); u->upsamplers.resize(n);
    out_ch = boc[n - 1];
    for (int i = 0; i < n; ++i) {
        const int prev_out = out_ch;
        out_ch = boc[n - 1 - i];
        const int in_ch = boc[n - 1 - std::min(i + 1, n - 1)];
        const int layers = cfg.layers_per_block + 1;
        u->up_res[i].resize(layers);
        if (cfg.up_attn[i]) u->up_attn[i].resize(layers);
        for (int j = 0; j < layers; ++j) {
            const int skip_ch = (j == layers - 1) ? in_ch : out_ch;
            const int res_in = (j == 0) ? prev_out : out_ch;
            const std::string base = "up_blocks." + std::to_string(i);
            add_resnet(u, u->up_res[i][j], base + ".resnets." + std::to_string(j), res_in + skip_ch, out_ch);
            if (cfg.up_attn[i]) add_attn(u, u->up_attn[i][j], base + ".attentions." + std::to_string(j), out_ch);
        }
        if (i != n - 1)
            add_conv(u, u->upsamplers[i], "up_blocks." + std::to_string(i) + ".upsamplers.0.conv", out_ch, out_ch, 3);
    }
    add_norm(u, u->norm_out, "conv_norm_out", boc[0]);
    add_conv(u, u->conv_out, "conv_out", cfg.out_channels, boc[0], 3);

    size_t off = 0;
    for (int64_t numel : u->dir.numels) {
        u->offsets.push_back(off);
        off += ((size_t)numel + 3) / 4 * 4;          // keep every tensor 16-byte aligned
    }
    u->raw_floats = off;
    return SISIC_OK;
}

// ------------------------------------------------------------------ derived weights
int prepare_conv(sisic_unet* u, ConvW& c, hipStream_t s) {
    SISIC_TRY(dev_alloc(u->owned, (size_t)sisic_conv_packed_numel(c.cout, c.cin, c.k), &c.packed));
    SISIC_TRY(launch_conv_pack(u->ctx, u->rawp(c.w_idx), c.cout, c.cin, c.k, c.packed, s));
    c.bias = u->rawp(c.b_idx);
    if (c.k == 3 && !c.strided && c.cout > 4) {
        SISIC_TRY(dev_alloc(u->owned, (size_t)winograd_packed_numel(c.cout, c.cin), &c.wino));
        SISIC_TRY(launch_winograd_pack(u->ctx, u->rawp(c.w_idx), c.cout, c.cin, c.wino, s));
    }
    if (c.k == 3 && c.strided) {
        SISIC_TRY(dev_alloc(u->owned, (size_t)conv_s2_packed_floats(c.cout, c.cin), &c.s2));
        SISIC_TRY(launch_conv_s2_pack(u->ctx, u->rawp(c.w_idx), c.cout, c.cin, c.s2, s));
    }
    return SISIC_OK;
}
void prepare_norm(sisic_unet* u, NormW& n) {
    n.gamma = u->rawp(n.w_idx);
    n.beta = u->rawp(n.b_idx);
}
// norms and the time-embedding projection (the block's convolutions: unet_prepare_all, with every other convolution)
int prepare_resnet(sisic_unet* u, ResnetW& r, hipStream_t s) {
    prepare_norm(u, r.norm1);
    prepare_norm(u, r.norm2);
    // time_emb_proj.weight [cout, hidden] -> columns [temb_off, temb_off+cout) of tproj_wt [hidden][R]
    SISIC_TRY(launch_transpose2d(u->ctx, u->rawp(r.temb_w_idx), r.cout, u->hidden, u->tproj_wt, u->tproj_R, r.temb_off, s));
    SISIC_HIP(hipMemcpyAsync(u->tproj_b + r.temb_off, u->rawp(r.temb_b_idx), (size_t)r.cout * sizeof(float), hipMemcpyDeviceToDevice, s));
    return SISIC_OK;
}
// the norm and q,k,v as one [3C, C] 1x1 convolution (to_out: unet_prepare_all, with every other convolution)
int prepare_attn(sisic_unet* u, AttnW& a, hipStream_t s) {
    prepare_norm(u, a.norm);
    const int c = a.c;
    SISIC_TRY(dev_alloc(u->owned, (size_t)3 * c * c, &a.qkv_cat));
    float* cat = a.qkv_cat;
    const size_t wbytes = (size_t)c * c * sizeof(float);
    SISIC_HIP(hipMemcpyAsync(cat, u->rawp(a.q_w), wbytes, hipMemcpyDeviceToDevice, s));
    SISIC_HIP(hipMemcpyAsync(cat + (size_t)c * c, u->rawp(a.k_w), wbytes, hipMemcpyDeviceToDevice, s));
    SISIC_HIP(hipMemcpyAsync(cat + (size_t)2 * c * c, u->rawp(a.v_w), wbytes, hipMemcpyDeviceToDevice, s));
    SISIC_TRY(dev_alloc(u->owned, (size_t)sisic_conv_packed_numel(3 * c, c, 1), &a.qkv_packed));
    SISIC_TRY(launch_conv_pack(u->ctx, cat, 3 * c, c, 1, a.qkv_packed, s));
    SISIC_TRY(dev_alloc(u->owned, (size_t)3 * c, &a.qkv_bias));
    SISIC_HIP(hipMemcpyAsync(a.qkv_bias, u->rawp(a.q_b), c * sizeof(float), hipMemcpyDeviceToDevice, s));
    SISIC_HIP(hipMemcpyAsync(a.qkv_bias + c, u->rawp(a.k_b), c * sizeof(float), hipMemcpyDeviceToDevice, s));
    SISIC_HIP(hipMemcpyAsync(a.qkv_bias + 2 * c, u->rawp(a.v_b), c * sizeof(float), hipMemcpyDeviceToDevice, s));
    return SISIC_OK;
}

// forget every derived buffer (they were freed): the next unet_prepare_all allocates afresh
void reset_derived(sisic_unet* u) {
    if (u->train) u->train->repack_ready = false;       // the job tables of repack.hip name the old buffers
    u->d_freqs = u->w1t = u->w2t = u->tproj_wt = u->tproj_b = nullptr;
    for (ConvW* c : unet_convs(u)) c->packed = c->wino = c->s2 = c->raw_t = c->packed_t = c->wino_t = nullptr;
    for (AttnW* a : unet_attns(u)) a->qkv_cat = a->qkv_packed = a->qkv_bias = a->qkv_raw_t = a->qkv_packed_t = nullptr;
}

// ------------------------------------------------------------------ workspace
void loop_graph_drop(sisic_unet* u) {
    if (u->loop_exec) (void)hipGraphExecDestroy(u->loop_exec);
    if (u->loop_graph) (void)hipGraphDestroy(u->loop_graph);
    u->loop_exec = nullptr; u->loop_graph = nullptr; u->loop_valid = false;
}

// A recorded training forward (the tape) owns pool blocks.  Whatever frees the pool, or lets a captured step write into
// blocks the tape took from the free list after the capture, makes the tape unusable: forget it, so that
// sisic_unet_backward answers SISIC_ESTATE instead of reading freed or overwritten activations.
void tape_forget(sisic_unet* u) {
    TrainState* tr = u->train.get();
    if (!tr) return;
    tr->bufs.clear();
    tr->grads_of_bufs.clear();
    tr->buf_grad.clear();
    tr->tape.clear();
    tr->has_tape = false;
}

void pool_release_all(sisic_unet* u) {
    loop_graph_drop(u);                 // a captured step holds addresses of pool blocks
    tape_forget(u);                     // ... and so does a recorded training forward
    u->pool.release_all();
}

}  // namespace

namespace sisic {

int unet_prepare_all(sisic_unet* u, hipStream_t s) {
    const int nin = 2 * u->cfg.n_freqs;
    SISIC_TRY(dev_alloc(u->owned, u->cfg.n_freqs, &u->d_freqs));
    SISIC_HIP(hipMemcpyAsync(u->d_freqs, u->freqs.data(), u->freqs.size() * sizeof(float), hipMemcpyHostToDevice, s));
    SISIC_TRY(dev_alloc(u->owned, (size_t)nin * u->hidden, &u->w1t));
    SISIC_TRY(dev_alloc(u->owned, (size_t)u->hidden * u->hidden, &u->w2t));
    SISIC_TRY(dev_alloc(u->owned, (size_t)u->hidden * u->tproj_R, &u->tproj_wt));
    SISIC_TRY(dev_alloc(u->owned, (size_t)u->tproj_R, &u->tproj_b));
    SISIC_TRY(launch_transpose2d(u->ctx, u->rawp(u->temb_w1), u->hidden, nin, u->w1t, u->hidden, 0, s));
    SISIC_TRY(launch_transpose2d(u->ctx, u->rawp(u->temb_w2), u->hidden, u->hidden, u->w2t, u->hidden, 0, s));
    prepare_norm(u, u->norm_out);
    for (ConvW* c : unet_convs(u)) SISIC_TRY(prepare_conv(u, *c, s));     // (to_out of every attention block included)
    for (ResnetW* r : unet_resnets(u)) SISIC_TRY(prepare_resnet(u, *r, s));
    for (AttnW* a : unet_attns(u)) SISIC_TRY(prepare_attn(u, *a, s));
    return SISIC_OK;
}

void unet_release_tape(sisic_unet* u) {
    if (TrainState* tr = u->train.get()) {
        for (auto& b : tr->bufs) {
            if (b->p) u->pool.put(b->p);
            if (b->stats) u->pool.put(b->stats);
        }
        for (float* p : tr->grads_of_bufs) u->pool.put(p);
    }
    tape_forget(u);
}

int unet_grow(float** p, size_t* have, size_t want) {
    if (*have >= want) return SISIC_OK;
    if (*p) SISIC_HIP(hipFree(*p));   // hipFree waits for the device, nothing can still read the old block
    *p = nullptr; *have = 0;
    void* q = nullptr;
    SISIC_HIP(hipMalloc(&q, want * sizeof(float)));
    SISIC_TRY(poison_fresh(q, want * sizeof(float)));
    *p = static_cast<float*>(q);
    *have = want;
    return SISIC_OK;
}

int unet_ensure_rows(sisic_unet* u, size_t t_rows, size_t gn_rows) {
    SISIC_TRY(unet_grow(&u->t_vals, &u->t_vals_cap, t_rows));
    SISIC_TRY(unet_grow(&u->temb_act, &u->temb_act_cap, t_rows * u->hidden));
    SISIC_TRY(unet_grow(&u->tproj, &u->tproj_cap, t_rows * u->tproj_R));
    SISIC_TRY(unet_grow(&u->gn_scale, &u->gn_scale_cap, gn_rows * u->max_c));
    SISIC_TRY(unet_grow(&u->gn_shift, &u->gn_shift_cap, gn_rows * u->max_c));
    SISIC_TRY(unet_grow(&u->gn_scale2, &u->gn_scale2_cap, gn_rows * u->max_c));
    SISIC_TRY(unet_grow(&u->gn_shift2, &u->gn_shift2_cap, gn_rows * u->max_c));
    return SISIC_OK;
}

// Host -> device upload of a few floats, ordered on the caller's stream.  The source is copied into
// one of a small ring of pinned slots; a slot is reused only after the copy that read it has finished.
int unet_stage_upload(sisic_unet* u, const float* src, size_t n, float* dst, hipStream_t s) {
    if (u->stage_cap < n) {
        SISIC_HIP(hipDeviceSynchronize());
        if (u->stage_host) SISIC_HIP(hipHostFree(u->stage_host));
        u->stage_host = nullptr;
        const size_t cap = std::max<size_t>(n, 1024);
        void* p = nullptr;
        SISIC_HIP(hipHostMalloc(&p, cap * sisic_unet::STAGE_SLOTS * sizeof(float), hipHostMallocDefault));
        u->stage_host = static_cast<float*>(p);
        u->stage_cap = cap;
        for (int i = 0; i < sisic_unet::STAGE_SLOTS; ++i) u->stage_used[i] = false;
    }
    const int slot = (int)(u->stage_next++ % sisic_unet::STAGE_SLOTS);
    if (!u->stage_ev[slot]) SISIC_HIP(hipEventCreateWithFlags(&u->stage_ev[slot], hipEventDisableTiming));
    if (u->stage_used[slot]) SISIC_HIP(hipEventSynchronize(u->stage_ev[slot]));
    float* h = u->stage_host + (size_t)slot * u->stage_cap;
    std::memcpy(h, src, n * sizeof(float));
    SISIC_HIP(hipMemcpyAsync(dst, h, n * sizeof(float), hipMemcpyHostToDevice, s));
    SISIC_HIP(hipEventRecord(u->stage_ev[slot], s));
    u->stage_used[slot] = true;
    return SISIC_OK;
}

int unet_check_labels(sisic_unet* u, const char* what, bool cond, const int64_t* labels, int B) {
    SISIC_REQUIRE(u, "%s: null handle", what);
    if (!cond) {
        SISIC_REQUIRE(u->n_class == 0, "%s: the model is class-conditional (sisic_unet_create_cond): call the _cond entry point with labels", what);
        return SISIC_OK;
    }
    SISIC_REQUIRE(u->n_class > 0, "%s: the model has no class embedding (sisic_unet_create): call the entry point without labels", what);
    SISIC_REQUIRE(labels && B > 0, "%s: null class_labels", what);
    for (int b = 0; b < B; ++b)
        SISIC_REQUIRE(labels[b] >= 0 && labels[b] < u->n_class, "%s: class_labels[%d] = %lld is outside [0, %d)", what, b,
                      (long long)labels[b], u->n_class);
    return SISIC_OK;
}

int unet_upload_labels(sisic_unet* u, const int64_t* labels, int B, float** dev, size_t* cap, hipStream_t s) {
    static_assert(sizeof(int) == sizeof(float), "labels are staged as floats");
    SISIC_TRY(unet_grow(dev, cap, (size_t)std::max(B, 64)));
    std::vector<float> bits(B);
    for (int b = 0; b < B; ++b) {
        const int v = (int)labels[b];
        std::memcpy(&bits[b], &v, sizeof(int));
    }
    return unet_stage_upload(u, bits.data(), (size_t)B, *dev, s);
}

int unet_check_shape(sisic_unet* u, int B, int H, int W) {
    SISIC_REQUIRE(u, "unet: null handle");
    if (!u->loaded) {
        set_error("unet: forward called before sisic_unet_load");
        return SISIC_ESTATE;
    }
    SISIC_HIP(hipSetDevice(u->ctx->device));
    const int div = 1 << (u->cfg.n_blocks - 1);
    SISIC_REQUIRE(B > 0 && H > 0 && W > 0 && H % div == 0 && W % div == 0,
                  "unet: sample %dx%dx%d unsupported (H and W must be positive multiples of %d)", B, H, W, div);
    if (u->ws_B != B || u->ws_H != H || u->ws_W != W) {
        SISIC_HIP(hipDeviceSynchronize());
        pool_release_all(u);
        u->ws_B = B; u->ws_H = H; u->ws_W = W;
    }
    return SISIC_OK;
}

}  // namespace sisic

namespace {

// ------------------------------------------------------------------ forward
// A tensor the executor reads or writes: where it is, its shape, and the pool buffer behind it.  buf is nullptr for the
// network's own input and output (as TapeOp means it); w, the pointer a convolution writes through, is nullptr for the
// network input, which is only read.
struct Act {
    const float* p = nullptr;
    float* w = nullptr;
    int C = 0, H = 0, W = 0;
    Buf* buf = nullptr;
    Act() = default;
    Act(Buf* b) : buf(b) { if (b) { p = w = b->p; C = b->C; H = b->H; W = b->W; } }
    Act(const float* in, int C_, int H_, int W_) : p(in), C(C_), H(H_), W(W_) {}
    Act(float* out, int C_, int H_, int W_) : p(out), w(out), C(C_), H(H_), W(W_) {}
};

// One convolution of the network: out = conv(act(cat(in0, in1))) + bias + chan_bias + residual
struct ConvOp {
    const ConvW* w = nullptr;
    Act in0, in1;                      // in1: the second tensor of a concatenation (empty: none)
    int stride = 1, ups = 0;           // ups: read in0 through a nearest-2x map
    bool gn_prologue = false;          // normalise the input with the pair the last gn() chose ...
    bool silu = false;                 // ... and apply SiLU
    const float* chan_bias = nullptr;  // per (sample, channel): this block's columns of the time-embedding projection
    Act residual, out;
    bool normed = false;               // a GroupNorm reads this output: have the epilogue leave partial statistics
    const NormW* next_norm = nullptr;  // ... and it is this one, reading the output ALONE: finalize it too where the launch can
    const AttnW* qkv_of = nullptr;     // the fused q/k/v projection of this attention block (tape)
    const GnFinJob* rider = nullptr;   // an independent GroupNorm finalisation the launch may carry; *carried: whether it did
    bool* carried = nullptr;
};

struct Fwd {
    sisic_unet* u;
    hipStream_t s;
    int B;
    const float* tproj;   // [B or 1, tproj_R]
    int tproj_stride;     // tproj_R, or 0 when one row serves every sample
    TrainState* tr = nullptr;     // training mode: record every operation, keep every buffer, save each GroupNorm's statistics
    PoolScope scope{u->pool, s};     // every block of bufs that is still out
    std::vector<std::unique_ptr<Buf>> bufs;
    float* gsc = u->gn_scale;     // scale / shift the next convolution's prologue reads (the shared pair, or this op's own)
    float* gsh = u->gn_shift;
    float* gmr = nullptr;         // training mode: (mean, rstd) of the same GroupNorm
    const NormW* gnorm = nullptr;
    int resnets_run = 0;          // ResNet blocks so far, in execution order: the block index of the dropout masks

    Buf* make(int C, int H, int W, int* rc) {
        auto b = std::make_unique<Buf>();
        b->C = C; b->H = H; b->W = W; b->refs = 1;
        *rc = scope.get((size_t)B * C * H * W, &b->p);
        bufs.push_back(std::move(b));
        return bufs.back().get();
    }
    void release(Buf* b) {
        if (tr) return;           // the backward pass reads every activation
        if (b && --b->refs == 0 && b->p) {
            scope.put(b->p);
            b->p = nullptr;
            if (b->stats) { scope.put(b->stats); b->stats = nullptr; }
        }
    }
    void advance(Buf*& x, Buf* y) { release(x); x = y; }

    // defer (inference only): where the finalisation would be a launch of its own, hand it back as a job instead -- the caller
    // has a neighbouring launch to carry it (resnet(): the shortcut) and runs it BEFORE anything reads the pair
    int gn(const Buf* x, const Buf* skip, const NormW& n, GnFinJob* defer = nullptr, bool* deferred = nullptr) {
        gsc = u->gn_scale; gsh = u->gn_shift; gmr = nullptr; gnorm = &n;
        if (!tr && !skip && x->fin_norm == static_cast<const void*>(&n)) {     // finalized by its producer (conv below)
            gsc = x->fin_scale; gsh = x->fin_shift;
            return SISIC_OK;
        }
        if (tr) {                 // this GroupNorm's own scale / shift / (mean, rstd): the backward pass needs them
            const int C = x->C + (skip ? skip->C : 0);
            SISIC_TRY(u->pool.get((size_t)B * C, &gsc, s));
            SISIC_TRY(u->pool.get((size_t)B * C, &gsh, s));
            SISIC_TRY(u->pool.get((size_t)B * u->cfg.norm_groups * 2, &gmr, s));
            tr->grads_of_bufs.push_back(gsc); tr->grads_of_bufs.push_back(gsh); tr->grads_of_bufs.push_back(gmr);
        }
        if (x->stats && (!skip || skip->stats)) { // every producer left partials: no pass over the tensors
            if (defer && !tr) {
                *deferred = true;
                return make_gn_fin_job(defer, x->stats, x->C, x->slots, skip ? skip->stats : nullptr, skip ? skip->C : 0,
                                       skip ? skip->slots : 0, B, u->cfg.norm_groups, u->cfg.norm_eps, n.gamma, n.beta, gsc, gsh);
            }
            return launch_gn_finalize(u->ctx, x->stats, x->C, x->slots, skip ? skip->stats : nullptr, skip ? skip->C : 0,
                                      skip ? skip->slots : 0, B, x->H * x->W, u->cfg.norm_groups, u->cfg.norm_eps,
                                      n.gamma, n.beta, gsc, gsh, s, gmr);
        }
        return launch_gn_stats(u->ctx, x->p, x->C, skip ? skip->p : nullptr, skip ? skip->C : 0, B, x->H * x->W,
                               u->cfg.norm_groups, u->cfg.norm_eps, n.gamma, n.beta, gsc, gsh, s, gmr);
    }

    int conv(const ConvOp& op) {
        const ConvW& c = *op.w;
        Buf* outb = op.out.buf;
        sisic_conv_args a{};
        a.in0 = op.in0.p; a.c0 = op.in0.C; a.in1 = op.in1.p; a.c1 = op.in1.C;
        a.B = B; a.Hin = op.in0.H; a.Win = op.in0.W; a.upsample = op.ups; a.ksize = c.k; a.stride = op.stride;
        a.w_packed = c.packed; a.bias = c.bias; a.Cout = c.cout;
        // (stride 2: the field carries the split filter of the bf16x3 downsampler kernel, sisic.h)
        a.w_winograd = op.stride == 1 ? (u->use_winograd ? c.wino : nullptr) : (op.stride == 2 ? c.s2 : nullptr);
        if (op.gn_prologue) { a.gn_scale = gsc; a.gn_shift = gsh; a.gn_silu = op.silu ? 1 : 0; }
        a.chan_bias = op.chan_bias; a.chan_bias_stride = tproj_stride;
        a.residual = op.residual.p; a.out = op.out.w;
        // single-image latency (the reference's own call pattern, image_generator.py:379: batch 1): conv_plan.cpp
        if (u->latency_mode) a.tile_cfg = conv_latency_cfg(a);
        if (op.normed && u->fuse_gn) {             // a GroupNorm reads this output: have the epilogue leave partials
            const int slots = conv_stats_slots(a);
            if (slots > 0) {
                SISIC_TRY(scope.get((size_t)B * c.cout * slots * 4, &outb->stats));
                outb->slots = slots;
                a.stats_out = outb->stats;
            }
        }
        // next_norm: the GroupNorm that reads this output ALONE, when the caller knows it: where the launch can finalize it
        // (sisic_conv_finalizes: the 8x8 level's K-split forms) it leaves that layer's (scale, shift) in the shared pair -- which
        // this very convolution's prologue may still be reading: the finalisation runs in the reduction launch behind it
        if (op.normed && op.next_norm && u->fuse_gn && !tr) {
            a.fin_gamma = op.next_norm->gamma; a.fin_beta = op.next_norm->beta; a.fin_groups = u->cfg.norm_groups; a.fin_eps = u->cfg.norm_eps;
            // (the pair this launch's own prologue is NOT reading: a workgroup finalizes its image while others still read theirs)
            const bool first_pair_busy = op.gn_prologue && gsc == u->gn_scale;
            a.fin_scale = first_pair_busy ? u->gn_scale2 : u->gn_scale;
            a.fin_shift = first_pair_busy ? u->gn_shift2 : u->gn_shift;
            if (conv_finalizes(a)) { outb->fin_norm = op.next_norm; outb->fin_scale = a.fin_scale; outb->fin_shift = a.fin_shift; }
            else { a.fin_gamma = nullptr; a.fin_beta = nullptr; a.fin_scale = nullptr; a.fin_shift = nullptr; }
        }
        if (tr) {
            TapeOp t;
            t.kind = TapeOp::CONV;
            t.w = c; t.qkv_of = op.qkv_of;
            t.in0 = op.in0.buf; t.in1 = op.in1.buf; t.in0_ptr = op.in0.p; t.in1_ptr = op.in1.p;
            t.c0 = op.in0.C; t.c1 = op.in1.C; t.H = op.in0.H; t.W = op.in0.W; t.stride = op.stride; t.ups = op.ups;
            if (op.gn_prologue) { t.norm = gnorm; t.gn_scale = gsc; t.gn_shift = gsh; t.gn_mr = gmr; t.silu = op.silu; }
            t.temb_off = op.chan_bias ? (int)(op.chan_bias - tproj) : -1;
            t.residual = op.residual.buf; t.out = outb; t.out_ptr = op.out.w;
            tr->tape.push_back(t);
        }
        return launch_conv2d(u->ctx, a, s, op.rider, op.carried);
    }

    // out = ResnetBlock2D(cat(x, skip)); consumes nothing (caller releases inputs)
    // next_norm: the GroupNorm module that reads the block's output alone, when the caller knows it (conv(): finalized by conv2's
    // own launch where that is possible)
    int resnet(const ResnetW& r, Buf* x, Buf* skip, Buf** out, const NormW* next_norm = nullptr) {
        int rc = SISIC_OK;
        const int H = x->H, W = x->W;
        const int c1 = skip ? skip->C : 0;
        SISIC_REQUIRE(x->C + c1 == r.cin, "unet: resnet expects %d input channels, got %d", r.cin, x->C + c1);
        // The 1x1 shortcut reads the raw block inputs only: it neither needs norm1 nor does conv1 need it.  In inference, where
        // norm1's finalisation would be a launch of its own, the shortcut runs FIRST and carries the jobs as extra workgroups
        // (conv_pointwise_bf3.hip); conv1, next in stream order, is the first reader of the pair.  The launcher says whether its
        // kernel ran them (the f32 1x1 kernels, latency mode's tiles and shapes the bf16x3 kernels refuse do not): if not, the
        // stand-alone launch follows.  (SISIC_GN_RIDER=0: the order and launches without any of this.)
        GnFinJob fin{};
        bool deferred = false;
        SISIC_TRY(gn(x, skip, r.norm1, (u->gn_rider && !tr && r.shortcut.k) ? &fin : nullptr, &deferred));
        Buf* sc = nullptr;
        auto shortcut = [&]() -> int {
            bool carried = false;
            sc = make(r.cout, H, W, &rc); SISIC_TRY(rc);
            ConvOp op;
            op.w = &r.shortcut; op.in0 = x; op.in1 = skip; op.out = sc;
            if (deferred) { op.rider = &fin; op.carried = &carried; }
            SISIC_TRY(conv(op));
            if (deferred && !carried) SISIC_TRY(launch_gn_finalize_job(u->ctx, fin, s));
            return SISIC_OK;
        };
        if (deferred) SISIC_TRY(shortcut());
        Buf* h = make(r.cout, H, W, &rc); SISIC_TRY(rc);
        {
            ConvOp op;
            op.w = &r.conv1; op.in0 = x; op.in1 = skip; op.gn_prologue = true; op.silu = true;
            op.chan_bias = tproj + r.temb_off; op.out = h; op.normed = true; op.next_norm = &r.norm2;
            SISIC_TRY(conv(op));
        }
        if (r.shortcut.k) {
            if (!deferred) SISIC_TRY(shortcut());
        } else {
            SISIC_REQUIRE(c1 == 0 && x->C == r.cout, "unet: identity shortcut with mismatched channels");
        }
        SISIC_TRY(gn(h, nullptr, r.norm2));
        // Dropout (a tape-recording forward with p > 0 only): h = conv2(dropout(silu(norm2(h)))).  One elementwise launch writes
        // the dropped activation, which stays on the tape -- conv2 and its weight gradient read it as a plain input
        const int block = resnets_run++;
        Buf* hd = nullptr;
        if (tr && tr->drop_p > 0.0f) {
            hd = make(r.cout, H, W, &rc); SISIC_TRY(rc);
            SISIC_TRY(launch_gn_silu_dropout(u->ctx, h->p, gsc, gsh, hd->p, B, r.cout, H * W, tr->drop_seed, tr->drop_call,
                                             256u + (uint32_t)block, tr->drop_p, tr->drop_inv_keep, s));
            TapeOp t;
            t.kind = TapeOp::DROPOUT;
            t.in0 = h; t.in0_ptr = h->p; t.c0 = r.cout; t.H = H; t.W = W;
            t.norm = &r.norm2; t.gn_scale = gsc; t.gn_shift = gsh; t.gn_mr = gmr; t.silu = true;
            t.out = hd; t.drop_block = block;
            tr->tape.push_back(t);
        }
        Buf* o = make(r.cout, H, W, &rc); SISIC_TRY(rc);
        {
            ConvOp op;
            op.w = &r.conv2; op.in0 = hd ? hd : h; op.gn_prologue = hd == nullptr; op.silu = hd == nullptr;
            op.residual = sc ? sc : x; op.out = o; op.normed = true; op.next_norm = next_norm;
            SISIC_TRY(conv(op));
        }
        release(hd);
        release(h);
        release(sc);
        *out = o;
        return SISIC_OK;
    }

    int attention(const AttnW& a, Buf* x, Buf** out) {
        int rc = SISIC_OK;
        const int H = x->H, W = x->W, N = H * W, C = a.c;
        SISIC_REQUIRE(x->C == C, "unet: attention channel mismatch");
        SISIC_TRY(gn(x, nullptr, a.norm));
        Buf* qkv = make(3 * C, H, W, &rc); SISIC_TRY(rc);
        ConvW cq; cq.cout = 3 * C; cq.cin = C; cq.k = 1; cq.packed = a.qkv_packed; cq.bias = a.qkv_bias;
        {
            ConvOp op;
            op.w = &cq; op.in0 = x; op.gn_prologue = true; op.out = qkv; op.qkv_of = &a;
            SISIC_TRY(conv(op));
        }
        Buf* o = make(C, H, W, &rc); SISIC_TRY(rc);
        SISIC_TRY(launch_attention(u->ctx, qkv->p, o->p, B, C, N, u->cfg.head_dim, s));
        if (tr) {
            TapeOp op;
            op.kind = TapeOp::ATTN;
            op.qkv = qkv; op.o = o; op.C = C; op.N = N;
            tr->tape.push_back(op);
        }
        release(qkv);
        Buf* y = make(C, H, W, &rc); SISIC_TRY(rc);
        {
            ConvOp op;
            op.w = &a.out; op.in0 = o; op.residual = x; op.out = y; op.normed = true;
            SISIC_TRY(conv(op));
        }
        release(o);
        *out = y;
        return SISIC_OK;
    }

    // a convolution between blocks (conv_in, the samplers): its output feeds a GroupNorm, nothing else is fused
    int plain_conv(const ConvW& c, const Act& in, int stride, int ups, Buf* out) {
        ConvOp op;
        op.w = &c; op.in0 = in; op.stride = stride; op.ups = ups; op.out = out; op.normed = true;
        return conv(op);
    }

    int run(const float* sample, float* out, int H, int W) {
        const sisic_unet_config& cfg = u->cfg;
        const int n = cfg.n_blocks;
        int rc = SISIC_OK;
        std::vector<Buf*> skips;

        Buf* x = make(u->conv_in.cout, H, W, &rc); SISIC_TRY(rc);
        SISIC_TRY(plain_conv(u->conv_in, Act(sample, cfg.in_channels, H, W), 1, 0, x));
        x->refs++;                 // held by `x` and by the skip stack
        skips.push_back(x);

        for (int i = 0; i < n; ++i) {
            for (int j = 0; j < cfg.layers_per_block; ++j) {
                Buf* y = nullptr;
                // who normalises this block's output next (alone: the up path's concatenations have two producers)
                const NormW* next = cfg.down_attn[i] ? &u->down_attn[i][j].norm
                                    : (j + 1 < cfg.layers_per_block ? &u->down_res[i][j + 1].norm1 : (i == n - 1 ? &u->mid_res[0].norm1 : nullptr));
                SISIC_TRY(resnet(u->down_res[i][j], x, nullptr, &y, next));
                advance(x, y);
                if (cfg.down_attn[i]) {
                    SISIC_TRY(attention(u->down_attn[i][j], x, &y));
                    advance(x, y);
                }
                x->refs++;
                skips.push_back(x);
            }
            if (i != n - 1) {
                const int Ho = (x->H + 2 - 3) / 2 + 1, Wo = (x->W + 2 - 3) / 2 + 1;
                Buf* y = make(u->downsamplers[i].cout, Ho, Wo, &rc); SISIC_TRY(rc);
                SISIC_TRY(plain_conv(u->downsamplers[i], x, 2, 0, y));
                advance(x, y);
                x->refs++;
                skips.push_back(x);
            }
        }

        {
            Buf* y = nullptr;
            SISIC_TRY(resnet(u->mid_res[0], x, nullptr, &y, &u->mid_attn.norm)); advance(x, y);
            SISIC_TRY(attention(u->mid_attn, x, &y)); advance(x, y);
            SISIC_TRY(resnet(u->mid_res[1], x, nullptr, &y)); advance(x, y);
        }

        for (int i = 0; i < n; ++i) {
            const int layers = cfg.layers_per_block + 1;
            for (int j = 0; j < layers; ++j) {
                SISIC_REQUIRE(!skips.empty(), "unet: skip stack underflow");
                Buf* skip = skips.back();
                skips.pop_back();
                SISIC_REQUIRE(skip->H == x->H && skip->W == x->W, "unet: skip resolution %dx%d vs %dx%d (H and W must be divisible by %d)",
                              skip->H, skip->W, x->H, x->W, 1 << (n - 1));
                Buf* y = nullptr;
                // (the block's output is normalised alone only when an attention block follows; the next ResNet block normalises
                //  it together with a skip tensor)
                SISIC_TRY(resnet(u->up_res[i][j], x, skip, &y, cfg.up_attn[i] ? &u->up_attn[i][j].norm : nullptr));
                advance(x, y);
                release(skip);
                if (cfg.up_attn[i]) {
                    SISIC_TRY(attention(u->up_attn[i][j], x, &y));
                    advance(x, y);
                }
            }
            if (i != n - 1) {
                Buf* y = make(u->upsamplers[i].cout, 2 * x->H, 2 * x->W, &rc); SISIC_TRY(rc);
                SISIC_TRY(plain_conv(u->upsamplers[i], x, 1, 1, y));
                advance(x, y);
            }
        }
        SISIC_REQUIRE(skips.empty(), "unet: skip stack not consumed");
        SISIC_REQUIRE(x->H == H && x->W == W, "unet: output resolution mismatch");
        SISIC_TRY(gn(x, nullptr, u->norm_out));
        ConvOp op;
        op.w = &u->conv_out; op.in0 = x; op.gn_prologue = true; op.silu = true; op.out = Act(out, cfg.out_channels, H, W);
        SISIC_TRY(conv(op));
        release(x);
        return SISIC_OK;
    }
};

// time embedding + all time_emb_proj rows for `rows` timesteps (t_vals already on the device); cond: plus the class embedding's
// row of each sample (u->labels_dev already on the device)
int time_embed(sisic_unet* u, int rows, hipStream_t s, bool cond = false) {
    SISIC_TRY(launch_temb_mlp(u->ctx, u->t_vals, rows, u->d_freqs, u->cfg.n_freqs, u->w1t, u->rawp(u->temb_b1), u->w2t,
                              u->rawp(u->temb_b2), u->hidden, u->temb_act, s, nullptr, nullptr, nullptr,
                              cond ? u->rawp(u->class_w) : nullptr, cond ? reinterpret_cast<const int*>(u->labels_dev) : nullptr));
    SISIC_TRY(launch_linear_t(u->ctx, u->temb_act, rows, u->hidden, u->tproj_wt, u->tproj_b, u->tproj_R, u->tproj, s));
    return SISIC_OK;
}

}  // namespace

int sisic::unet_run_forward(sisic_unet* u, const float* sample, const float* tproj, int tproj_stride, float* out, int B, int H,
                            int W, hipStream_t s, TrainState* tr) {
    Fwd f{u, s, B, tproj, tproj_stride, tr};
    const int rc = f.run(sample, out, H, W);      // inference, and error paths: f.scope hands everything back
    if (tr && rc == SISIC_OK) {                   // training mode: the tape owns the activations until the backward pass has run
        for (auto& b : f.bufs) tr->bufs.push_back(std::move(b));
        f.scope.disown();
    } else if (tr) {
        tr->tape.clear();
    }
    return rc;
}

extern "C" {

int sisic_unet_create(sisic_ctx* ctx, const sisic_unet_config* cfg, sisic_unet** out) {
    return sisic_unet_create_cond(ctx, cfg, 0, out);
}

int sisic_unet_create_cond(sisic_ctx* ctx, const sisic_unet_config* cfg, int num_class_embeds, sisic_unet** out) {
    SISIC_REQUIRE(ctx && cfg && out, "unet_create: null argument");
    *out = nullptr;
    SISIC_REQUIRE(num_class_embeds >= 0, "unet_create: num_class_embeds %d", num_class_embeds);
    SISIC_REQUIRE(cfg->n_blocks >= 1 && cfg->n_blocks <= 8, "unet_create: n_blocks %d", cfg->n_blocks);
    SISIC_REQUIRE(cfg->layers_per_block >= 1, "unet_create: layers_per_block");
    SISIC_REQUIRE(cfg->in_channels > 0 && cfg->out_channels > 0, "unet_create: channels");
    SISIC_REQUIRE(cfg->norm_groups > 0, "unet_create: norm_groups %d", cfg->norm_groups);
    SISIC_REQUIRE(cfg->head_dim == 8 || cfg->head_dim == 32 || cfg->head_dim == 64,
                  "unet_create: head_dim %d is not one of 8, 32, 64 (the widths the attention kernels are built for)", cfg->head_dim);
    SISIC_REQUIRE(cfg->freqs && cfg->n_freqs * 2 == cfg->block_out_channels[0], "unet_create: freqs table must hold block_out_channels[0]/2 entries");
    for (int i = 0; i < cfg->n_blocks; ++i) {
        SISIC_REQUIRE(cfg->block_out_channels[i] > 0 && cfg->block_out_channels[i] % cfg->norm_groups == 0,
                      "unet_create: block_out_channels[%d]=%d", i, cfg->block_out_channels[i]);
        // (head_dim 8 keeps its rule for every width; at 32 and 64 only the widths that carry attention: down block i, up block
        //  n-1-i and, at the lowest level, the mid block)
        const bool attn = cfg->down_attn[i] || cfg->up_attn[cfg->n_blocks - 1 - i] || i == cfg->n_blocks - 1;
        SISIC_REQUIRE((cfg->head_dim != 8 && !attn) || cfg->block_out_channels[i] % cfg->head_dim == 0,
                      "unet_create: block_out_channels[%d]=%d is no multiple of head_dim %d", i, cfg->block_out_channels[i],
                      cfg->head_dim);
    }
    auto* u = new sisic_unet();
    u->ctx = ctx;
    u->cfg = *cfg;
    u->freqs.assign(cfg->freqs, cfg->freqs + cfg->n_freqs);
    if (const char* e = std::getenv("SISIC_WINOGRAD")) u->use_winograd = std::atoi(e) != 0;
    if (const char* e = std::getenv("SISIC_FUSED_GN")) u->fuse_gn = std::atoi(e) != 0;
    if (const char* e = std::getenv("SISIC_GN_RIDER")) u->gn_rider = std::atoi(e) != 0;
    if (const char* e = std::getenv("SISIC_GRAPH")) u->graph_mode = std::atoi(e) != 0 ? 1 : 0;
    if (poison_alloc()) u->graph_mode = 0;
    u->cfg.freqs = nullptr;
    u->n_class = num_class_embeds;
    const int rc = describe(u);
    if (rc != SISIC_OK) { delete u; return rc; }
    *out = u;
    return SISIC_OK;
}

int sisic_unet_destroy(sisic_unet* u) {
    if (!u) return SISIC_OK;
    (void)sisic_unet_train_end(u);
    (void)hipDeviceSynchronize();
    pool_release_all(u);
    for (float* p : {u->x_work, u->loop_tables, u->tproj_cur, u->seeds_dev, u->hist_buf, u->cond_tables, u->edit_x0k, u->edit_mask,
                     u->edit_rows, u->objective_dev, u->clf_grad, u->clf_tables, u->thr_s})
        if (p) (void)hipFree(p);
    if (u->loop_stream) (void)hipStreamDestroy(u->loop_stream);
    for (auto p : u->owned) (void)hipFree(p);
    for (float* p : {u->raw, u->t_vals, u->temb_act, u->tproj, u->gn_scale, u->gn_shift, u->gn_scale2, u->gn_shift2, u->eps_buf,
                     u->labels_dev})
        if (p) (void)hipFree(p);
    if (u->stage_host) (void)hipHostFree(u->stage_host);
    for (auto e : u->stage_ev)
        if (e) (void)hipEventDestroy(e);
    delete u;
    return SISIC_OK;
}

int sisic_unet_set_latency_mode(sisic_unet* u, int on) {
    SISIC_REQUIRE(u, "set_latency_mode: null handle");
    u->latency_mode = on != 0;
    return SISIC_OK;
}

int sisic_unet_set_graph_mode(sisic_unet* u, int mode) {
    SISIC_REQUIRE(u && mode >= -1 && mode <= 1, "set_graph_mode: mode must be -1 (follow latency mode), 0 or 1");
    u->graph_mode = mode;
    return SISIC_OK;
}

int64_t sisic_unet_graph_builds(const sisic_unet* u) { return u ? u->loop_builds : 0; }

int sisic_unet_set_prediction_type(sisic_unet* u, int type) {
    SISIC_REQUIRE(u, "set_prediction_type: null handle");
    SISIC_REQUIRE(type == SISIC_PRED_EPSILON || type == SISIC_PRED_SAMPLE || type == SISIC_PRED_V,
                  "set_prediction_type: type %d (0 = epsilon, 1 = sample, 2 = v)", type);
    u->pred_type = type;
    return SISIC_OK;
}

int sisic_unet_prediction_type(const sisic_unet* u) { return u ? u->pred_type : SISIC_PRED_EPSILON; }

int sisic_unet_set_thresholding(sisic_unet* u, float ratio, float sample_max_value) {
    SISIC_REQUIRE(u, "set_thresholding: null handle");
    SISIC_TRY(check_thresholding("set_thresholding", ratio, sample_max_value));
    u->thr_ratio = ratio > 0.0f ? ratio : 0.0f;
    u->thr_max = sample_max_value;
    return SISIC_OK;
}

int64_t sisic_unet_workspace_bytes(const sisic_unet* u) {
    return u ? u->pool.bytes() : 0;
}

int sisic_unet_num_tensors(const sisic_unet* u) { return u ? u->dir.size() : 0; }

const char* sisic_unet_tensor_name(const sisic_unet* u, int i) { return u ? u->dir.name(i) : nullptr; }

int sisic_unet_load(sisic_unet* u, int n, const char* const* names, const float* const* host_ptrs,
                    const int64_t* numels) {
    SISIC_REQUIRE(u && names && host_ptrs && numels, "unet_load: null argument");
    std::vector<int> slot;                    // a refused state dict leaves the handle as it was: nothing below has run
    SISIC_TRY(u->dir.match("unet_load", n, names, host_ptrs, numels, &slot));
    SISIC_HIP(hipSetDevice(u->ctx->device));
    if (!u->raw) SISIC_HIP(hipMalloc(&u->raw, u->raw_floats * sizeof(float)));
    SISIC_HIP(hipMemset(u->raw, 0, u->raw_floats * sizeof(float)));
    for (int i = 0; i < n; ++i)
        SISIC_HIP(hipMemcpy(u->raw + u->offsets[slot[i]], host_ptrs[i], (size_t)numels[i] * sizeof(float), hipMemcpyHostToDevice));
    // (re)build derived buffers.  A captured sampling step holds the addresses of the packed filters freed below: drop it
    // (a replay after load_state_dict would read freed memory).
    SISIC_HIP(hipDeviceSynchronize());
    loop_graph_drop(u);
    for (auto p : u->owned) (void)hipFree(p);
    u->owned.clear();
    reset_derived(u);
    u->loaded = false;
    SISIC_TRY(unet_prepare_all(u, nullptr));
    SISIC_HIP(hipDeviceSynchronize());
    u->loaded = true;
    return SISIC_OK;
}

// labels: host int64 [B] of a conditional model (checked by the caller), or nullptr
static int forward_impl(sisic_unet* u, const float* sample, const int64_t* timesteps, const int64_t* labels, float* out, int B,
                        int H, int W, hipStream_t s) {
    SISIC_TRY(unet_check_shape(u, B, H, W));
    SISIC_TRY(unet_ensure_rows(u, (size_t)B, (size_t)B));
    std::vector<float> tv(B);
    bool uniform = true;      // one embedding row serves every sample: equal timesteps and, with labels, equal labels
    for (int b = 0; b < B; ++b) {
        tv[b] = (float)timesteps[b];
        uniform = uniform && timesteps[b] == timesteps[0] && (!labels || labels[b] == labels[0]);
    }
    const int rows = uniform ? 1 : B;
    SISIC_TRY(unet_stage_upload(u, tv.data(), (size_t)rows, u->t_vals, s));
    if (labels) SISIC_TRY(unet_upload_labels(u, labels, rows, &u->labels_dev, &u->labels_cap, s));
    SISIC_TRY(time_embed(u, rows, s, labels != nullptr));
    return unet_run_forward(u, sample, u->tproj, uniform ? 0 : u->tproj_R, out, B, H, W, s);
}

int sisic_unet_forward(sisic_unet* u, const float* sample, const int64_t* timesteps, float* out, int B, int H, int W,
                       void* stream) {
    SISIC_REQUIRE(u && sample && timesteps && out, "unet_forward: null argument");
    SISIC_TRY(unet_check_labels(u, "unet_forward", false, nullptr, B));
    return forward_impl(u, sample, timesteps, nullptr, out, B, H, W, static_cast<hipStream_t>(stream));
}

int sisic_unet_forward_cond(sisic_unet* u, const float* sample, const int64_t* timesteps, const int64_t* class_labels,
                            float* out, int B, int H, int W, void* stream) {
    SISIC_REQUIRE(u && sample && timesteps && out, "unet_forward_cond: null argument");
    SISIC_TRY(unet_check_labels(u, "unet_forward_cond", true, class_labels, B));
    return forward_impl(u, sample, timesteps, class_labels, out, B, H, W, static_cast<hipStream_t>(stream));
}

// the device tables of the replayed loop: 1000 rows of the widest rule's coefficients (a rule's rows lie packed at its own
// width from the start of the region), then the noise row of each step
static constexpr size_t LOOP_COEF_FLOATS = 6 * 1000;
static constexpr size_t LOOP_TABLE_FLOATS = 4 + LOOP_COEF_FLOATS + 1000;

// A conditional call of the loop (sisic_sample_frames_cond): every sample of a pass has its own embedding row, and a guided
// call runs each pass at twice the batch
struct CondCall {
    bool guided = false;     // guidance_scale != 1: conditional rows first, null-label rows second, combined in the step kernel
    int rows = 0;            // samples per UNet pass: B, or 2B when guided
    float w = 1.0f;
};

// An edited call of the loop (sisic_sample_frames_edit): the known image, the mask (both device) and the host edit rows [T][4]
struct EditCall {
    const float* x0k;
    const float* mask;
    const float* rows;
};
static constexpr size_t LOOP_EDIT_FLOATS = 4 * 1000;

// A classifier-guided call of the loop (sisic_sample_frames_clf): the classifier, the images' targets (host) and the scale
struct ClfCall {
    sisic_resnet* clf;
    const int64_t* targets;
    float scale;
};

// One call of the sampling loop as its public entry point describes it (sisic.h): what every form of the loop is given.
struct LoopCall {
    float* x = nullptr;
    int B = 0, H = 0, W = 0, T = 0;
    const int64_t* timesteps = nullptr;
    const float* coef = nullptr;
    float clip = 0.0f;
    int rule = SISIC_RULE_DDPM, rule_flags = 0;     // (sample_frames adds the handle's prediction type to the flags)
    const float* noise = nullptr;                   // the noise buffer of sisic_sample_frames[_rule], or
    const uint64_t* seeds = nullptr;                // HOST uint64 [B]: the step generates its noise, step index step0 + i
    int step0 = 0;
    const int64_t* labels = nullptr;                // sisic_sample_frames_cond: host int64 [B], with null_label and the scale w
    int null_label = 0;
    float w = 1.0f;
    const EditCall* ed = nullptr;
    const ClfCall* cl = nullptr;
    float* traj = nullptr;
    const int* traj_row = nullptr;
    uint8_t* out_u8 = nullptr;
    const volatile int* cancel = nullptr;
    int* steps_done = nullptr;
    void* stream = nullptr;
    const CondCall* cg = nullptr;                   // set by sample_frames for a conditional call
};

// The step launch of a call (common.h StepLaunch) on the latent x.  i >= 0: the eager form of step i, with its host row, its
// step index, w and its noise row z.  i < 0: the replayed form, which reads all of these by the loop's step from the device
// tables (and the library's copies of an edited call's image, mask and rows: a captured step serves every edited call at the
// shape).
static StepLaunch loop_step_launch(const sisic_unet* u, const LoopCall& c, float* x, size_t n, int i, const float* z) {
    const bool guided = c.cg && c.cg->guided;
    StepLaunch L;
    L.rule = c.rule; L.flags = c.rule_flags; L.clip = c.clip;
    L.source = c.cl ? STEP_EPS_CLASSIFIER : guided ? STEP_EPS_GUIDED : STEP_EPS_PLAIN;
    L.eps = u->eps_buf;
    if (guided) L.eps_u = u->eps_buf + n;
    if (c.cl) L.grad = u->clf_grad;
    L.x = x; L.out = x; L.n = (int64_t)n;
    if (c.rule == STEP_RULE_DPMPP) L.hist = u->hist_buf;
    L.device_noise = c.seeds != nullptr;
    if (c.seeds) L.seeds_dev = reinterpret_cast<const uint64_t*>(u->seeds_dev);
    L.n_per_image = (int64_t)(n / c.B);
    // (the handle's thresholding: sample_frames has sized thr_s; the quantile launch is launch_step's first)
    if (u->thr_ratio > 0.0f) { L.thr_s = u->thr_s; L.thr_ratio = u->thr_ratio; L.thr_max = u->thr_max; }
    L.edit = c.ed != nullptr;
    L.hw = (int64_t)c.H * c.W;
    if (i >= 0) {
        L.row = c.coef + (size_t)i * SISIC_RULE_ROW_WIDTH(c.rule);
        L.z = z;
        L.step = (uint32_t)(c.step0 + i);
        L.w = c.cl ? c.cl->scale : guided ? c.cg->w : 1.0f;
        if (c.ed) { L.x0k = c.ed->x0k; L.mask = c.ed->mask; L.erow = c.ed->rows + 4 * (size_t)i; }
    } else {
        L.state = u->loop_tables;
        L.coef_dev = u->loop_tables + 4;
        L.zrow_dev = reinterpret_cast<const int*>(u->loop_tables + 4 + LOOP_COEF_FLOATS);
        L.w_tab = c.cl ? u->clf_tables : guided ? u->cond_tables : nullptr;
        if (c.ed) { L.x0k = u->edit_x0k; L.mask = u->edit_mask; L.erows_dev = u->edit_rows; }
    }
    return L;
}

// One denoising step with every per-step parameter selected on the device (elementwise.hip, LoopState): identical
// launches for every step, so that a captured step can be replayed.  A classifier-guided call runs the classifier's gradient
// walk between the UNet pass and the step kernel.
static int loop_step(sisic_unet* u, const LoopCall& c, size_t n, hipStream_t s) {
    void* state = u->loop_tables;
    if (c.cg) {
        SISIC_TRY(launch_loop_gather_rows(u->ctx, u->tproj, u->tproj_R, state, 0, u->cond_tables, c.cg->rows, u->tproj_cur, s));
        SISIC_TRY(unet_run_forward(u, u->x_work, u->tproj_cur, u->tproj_R, u->eps_buf, c.cg->rows, c.H, c.W, s));
    } else {
        SISIC_TRY(launch_loop_select_row(u->ctx, u->tproj, u->tproj_R, state, u->tproj_cur, s));
        SISIC_TRY(unet_run_forward(u, u->x_work, u->tproj_cur, 0, u->eps_buf, c.B, c.H, c.W, s));
    }
    // the walk on the loop's latent, on the loop's stream, behind the UNet pass; targets and scale from the loop's table
    if (c.cl)
        SISIC_TRY(resnet_input_gradient_walk(c.cl->clf, u->x_work, c.B, c.H, c.W, 0,
                                             reinterpret_cast<const int*>(u->clf_tables + LOOP_CLF_HEAD), u->clf_grad, nullptr, s));
    SISIC_TRY(launch_step(u->ctx, loop_step_launch(u, c, u->x_work, n, -1, nullptr), s));
    return launch_loop_advance(u->ctx, state, s);
}

// Step i of the eager form on the latent xs: the UNet pass under the step's own embedding rows, the classifier's walk of a
// classifier-guided call, then the step kernel with the host row and the next unused noise row (*zi counts them).
static int eager_step(sisic_unet* u, const LoopCall& c, float* xs, size_t n, hipStream_t s, int i, size_t* zi) {
    if (c.cg) {
        SISIC_TRY(launch_loop_gather_rows(u->ctx, u->tproj, u->tproj_R, nullptr, i, u->cond_tables, c.cg->rows, u->tproj_cur, s));
        SISIC_TRY(unet_run_forward(u, xs, u->tproj_cur, u->tproj_R, u->eps_buf, c.cg->rows, c.H, c.W, s));
    } else {
        SISIC_TRY(unet_run_forward(u, xs, u->tproj + (size_t)i * u->tproj_R, 0, u->eps_buf, c.B, c.H, c.W, s));
    }
    const float* z = nullptr;
    if (c.noise && c.coef[(size_t)i * SISIC_RULE_ROW_WIDTH(c.rule) + 4] != 0.0f) z = c.noise + ((*zi)++) * n;
    if (c.cl)
        SISIC_TRY(resnet_input_gradient_walk(c.cl->clf, xs, c.B, c.H, c.W, 0, reinterpret_cast<const int*>(u->clf_tables + LOOP_CLF_HEAD),
                                             u->clf_grad, nullptr, s));
    return launch_step(u->ctx, loop_step_launch(u, c, xs, n, i, z), s);
}

// The replayed form: the loop as ONE captured step replayed T-1 times (hipGraph): at batch 1 a step is ~190 launches of 5-20 us
// kernels and the host cannot issue them as fast as the GPU retires them (measured: 3.0 ms of kernels in a 4.5 ms step).
// A call with seeds generates its noise from u->seeds_dev (already uploaded on the caller's stream) with step index step0 + i.
//
// What it sets up before the loop: the stream the steps run on (*sp), the device tables of the call, the library's copies of an
// edited call's image, mask and rows, and the call's latent in x_work (every address inside the graph is library-owned).
static int replay_begin(sisic_unet* u, const LoopCall& c, size_t n, hipStream_t* sp) {
    const bool rng = c.seeds != nullptr;
    const size_t cw = SISIC_RULE_ROW_WIDTH(c.rule);
    SISIC_REQUIRE(c.T <= 1000, "sample: at most 1000 steps per call");
    // the replayed launches write into the pool blocks they were captured with; a tape recorded since then may own some of
    // them: the tape does not survive a graph-replayed run (sisic_unet_backward then answers SISIC_ESTATE)
    unet_release_tape(u);
    if (!*sp) {                            // the legacy default stream cannot be captured: a blocking stream of our own,
        if (!u->loop_stream) SISIC_HIP(hipStreamCreate(&u->loop_stream));     // implicitly ordered with the default stream
        *sp = u->loop_stream;
    }
    hipStream_t s = *sp;
    const bool guided = c.cg && c.cg->guided;
    // (a guided call keeps the latent twice, one copy per half of the batch the UNet runs; the step kernel writes both)
    SISIC_TRY(unet_grow(&u->x_work, &u->x_work_cap, guided ? 2 * n : n));
    SISIC_TRY(unet_grow(&u->tproj_cur, &u->tproj_cur_cap, (size_t)(c.cg ? c.cg->rows : 1) * u->tproj_R));
    SISIC_TRY(unet_grow(&u->loop_tables, &u->loop_tables_cap, LOOP_TABLE_FLOATS));
    // tables of this call: {step = 0, step base, noise base}, coefficients, noise row per step (-1: the step adds no noise)
    std::vector<float> tab(LOOP_TABLE_FLOATS, 0.0f);
    {
        const int first = 0, base = rng ? c.step0 : 0;
        std::memcpy(&tab[0], &first, sizeof(int));
        std::memcpy(&tab[1], &base, sizeof(int));
        std::memcpy(&tab[2], &c.noise, sizeof(c.noise));
        std::memcpy(&tab[4], c.coef, (size_t)c.T * cw * sizeof(float));
        int* zr = reinterpret_cast<int*>(&tab[4 + LOOP_COEF_FLOATS]);
        int zi = 0;
        for (int i = 0; i < c.T; ++i) zr[i] = (c.noise && c.coef[(size_t)i * cw + 4] != 0.0f) ? zi++ : -1;
    }
    SISIC_TRY(unet_stage_upload(u, tab.data(), tab.size(), u->loop_tables, s));
    if (c.ed) {
        const size_t nm = (size_t)c.B * c.H * c.W;
        SISIC_TRY(unet_grow(&u->edit_x0k, &u->edit_x0k_cap, n));
        SISIC_TRY(unet_grow(&u->edit_mask, &u->edit_mask_cap, nm));
        SISIC_TRY(unet_grow(&u->edit_rows, &u->edit_rows_cap, LOOP_EDIT_FLOATS));
        SISIC_HIP(hipMemcpyAsync(u->edit_x0k, c.ed->x0k, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        SISIC_HIP(hipMemcpyAsync(u->edit_mask, c.ed->mask, nm * sizeof(float), hipMemcpyDeviceToDevice, s));
        SISIC_TRY(unet_stage_upload(u, c.ed->rows, (size_t)c.T * 4, u->edit_rows, s));
    }
    SISIC_HIP(hipMemcpyAsync(u->x_work, c.x, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    if (guided) SISIC_HIP(hipMemcpyAsync(u->x_work + n, c.x, n * sizeof(float), hipMemcpyDeviceToDevice, s));
    return SISIC_OK;
}

// The key of the captured step that the call (u, c) on stream s replays (unet_internal.h says why each field is there), from the
// handle as it stands: read before step 0 and again behind it, because the eager step sizes the pool and the scratch buffers.
static sisic_unet::LoopKey loop_key_of(const sisic_unet* u, const LoopCall& c, hipStream_t s) {
    sisic_unet::LoopKey k;
    k.B = c.B; k.H = c.H; k.W = c.W; k.clip = c.clip; k.s = s; k.latency = u->latency_mode;
    k.gen = u->ctx->scratch_generation.load();
    // every address baked into the captured launches: the pool and the scratch buffers are sized by the first eager step at a
    // shape, the tables by ensure_rows / grow, hist_buf and thr_s by sample_frames before the loop
    const void* ptrs[] = {u->tproj, u->eps_buf, u->x_work, u->loop_tables, u->tproj_cur,
                          c.rule == STEP_RULE_DPMPP ? u->hist_buf : nullptr, c.cg ? u->cond_tables : nullptr,
                          c.ed ? u->edit_x0k : nullptr, c.ed ? u->edit_mask : nullptr, c.ed ? u->edit_rows : nullptr,
                          c.cl ? u->clf_grad : nullptr, c.cl ? u->clf_tables : nullptr, u->thr_ratio > 0.0f ? u->thr_s : nullptr};
    static_assert(sizeof(ptrs) == sizeof(k.ptrs), "LoopKey::ptrs holds every address of the list");
    std::copy(std::begin(ptrs), std::end(ptrs), k.ptrs);
    // (labels and the guidance scale live in cond_tables and change nothing a captured launch holds; whether the call is
    //  conditional, and whether it is guided, change the launches themselves)
    k.cond = c.cg != nullptr; k.guided = c.cg && c.cg->guided; k.edit = c.ed != nullptr;
    k.thr_ratio = u->thr_ratio; k.thr_max = u->thr_max;
    // (a classifier-guided call: targets and scale live in clf_tables; the classifier's own blocks and weight buffers are
    //  covered by the generation of its workspace)
    k.clf = c.cl != nullptr;
    k.clf_handle = c.cl ? c.cl->clf : nullptr;
    k.clf_gen = c.cl ? resnet_workspace_generation(c.cl->clf) : 0;
    k.rng = c.seeds != nullptr;
    k.seeds = k.rng ? u->seeds_dev : nullptr;
    k.rule = c.rule; k.rule_flags = c.rule_flags;
    return k;
}

// Step i of the replayed form.  Until the call has its graph (*ready): a call that finds it replays from step 0; one that does
// not runs step 0 eagerly (loop_step: sizes the pool and every scratch buffer, opts the kernels in to their LDS sizes -- ~190
// launches, twice the time of a replayed step at batch 1) and captures before its first replay.
static int replay_step(sisic_unet* u, const LoopCall& c, size_t n, hipStream_t s, int i, bool* ready) {
    if (!*ready) {
        const sisic_unet::LoopKey want = loop_key_of(u, c, s);
        if (!(u->loop_valid && want == u->loop_key)) {
            if (i == 0) return loop_step(u, c, n, s);
            loop_graph_drop(u);
            SISIC_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeRelaxed));
            const int crc = loop_step(u, c, n, s);
            hipGraph_t g = nullptr;
            const hipError_t e = hipStreamEndCapture(s, &g);
            if (crc != SISIC_OK || e != hipSuccess || !g) {
                if (g) (void)hipGraphDestroy(g);
                if (crc == SISIC_OK) set_error("sample: stream capture failed: %s", hipGetErrorString(e));
                return crc != SISIC_OK ? crc : SISIC_EHIP;
            }
            u->loop_graph = g;
            SISIC_HIP(hipGraphInstantiate(&u->loop_exec, g, nullptr, nullptr, 0));
            u->loop_key = want;
            u->loop_valid = true;
            u->loop_builds += 1;
        }
        *ready = true;
    }
    SISIC_HIP(hipGraphLaunch(u->loop_exec, s));
    return SISIC_OK;
}

// The loop behind sisic_sample_frames[_rule] (noise: a buffer or NULL; seeds NULL) and sisic_sample_frames[_rule]_rng (seeds:
// HOST uint64 [B], noise NULL): the two differ in where the scheduler step takes z from, nothing else.  rule, rule_flags: the
// step rule whose rows coef holds (SISIC_RULE_*).  labels: sisic_sample_frames_cond (host int64 [B], with null_label and the
// guidance scale w), or nullptr for an unconditional handle.  (c: this function's own copy, which gains the prediction type in
// its flags and the conditional call's rows.)
//
// One loop over the steps with two forms of "run step i": eager_step, today's launches with the host row, and replay_step, the
// captured step.  Each form sets up what it needs before the loop; the poll of the stop flag, the trajectory copy, steps_done
// and everything behind the loop are the same for both.
static int sample_frames(sisic_unet* u, LoopCall c) {
    SISIC_REQUIRE(u && c.x && c.timesteps && c.coef && c.T > 0, "sample: null argument");
    const int B = c.B, H = c.H, W = c.W, T = c.T;
    // a caller's flags are the rule's own; from here on c.rule_flags also carries the handle's prediction type in its private
    // bits, down to the launchers and into the key of a captured step
    SISIC_REQUIRE((c.rule_flags & ~SISIC_RULE_FLAG_CLIPPED_OUTPUT) == 0, "sample: rule flags %d (SISIC_RULE_FLAG_CLIPPED_OUTPUT or 0)",
                  c.rule_flags);
    c.rule_flags |= step_pred_flags(u->pred_type);
    SISIC_TRY(unet_check_labels(u, c.labels ? "sample_cond" : "sample", c.labels != nullptr, c.labels, B));
    SISIC_REQUIRE(!c.traj_row || c.traj, "sample: traj_row without a trajectory buffer");
    if (c.traj_row)
        for (int i = 0; i < T; ++i) SISIC_REQUIRE(c.traj_row[i] >= -1, "sample: traj_row[%d] = %d (a row of traj, or -1)", i, c.traj_row[i]);
    hipStream_t s = static_cast<hipStream_t>(c.stream);
    if (c.steps_done) *c.steps_done = 0;
    // the eager DDPM step checks its divisor launch by launch, as it always has; a rule chosen by the caller is checked for
    // the whole table before the first launch (the replayed step reads its row on the device and cannot refuse it)
    const size_t cw = SISIC_RULE_ROW_WIDTH(c.rule);      // (an unknown rule is refused by check_step_row just below)
    if (c.rule != STEP_RULE_DDPM || c.rule_flags != 0 || c.labels || c.ed || c.cl)
        for (int i = 0; i < T; ++i)
            SISIC_TRY(check_step_row(c.rule, c.rule_flags, c.coef[(size_t)i * cw + 0], c.coef[(size_t)i * cw + 1]));
    // DPM-Solver++: a call starts with no history (the buffer holds whatever the last run left), so its first step cannot be
    // a second-order one.  A run cut into two calls therefore differs from the uncut run; callers run it in one call.
    if (c.rule == STEP_RULE_DPMPP)
        SISIC_REQUIRE(c.coef[5] == 0.0f, "sample: row 0 of a DPM-Solver++ call has k1 = %g (a call starts with no history)", c.coef[5]);
    if (c.ed) {
        // the replayed step reads its edit row on the device and cannot refuse it: the whole table is checked here
        SISIC_REQUIRE(c.seeds && c.ed->x0k && c.ed->mask && c.ed->rows, "sample_edit: null argument (the known image, the mask, the edit rows and the seeds are required)");
        SISIC_REQUIRE(T <= 1000, "sample_edit: at most 1000 steps per call");
        for (int i = 0; i < T; ++i) {
            const float* r = c.ed->rows + 4 * (size_t)i;
            SISIC_REQUIRE(std::isfinite(r[0]) && std::isfinite(r[1]) && std::isfinite(r[2]) && std::isfinite(r[3]),
                          "sample_edit: edit row %d is {%g, %g, %g, %g}", i, r[0], r[1], r[2], r[3]);
            SISIC_REQUIRE(c.rule != STEP_RULE_DPMPP || r[3] == 0.0f,
                          "sample_edit: edit row %d jumps (jb = %g) under DPM-Solver++: a jump invalidates the history", i, r[3]);
        }
    }
    // a conditional call: the distinct labels of the call (in order of first appearance, the null one last when guided) are the
    // slots of the embedding table; sample b of a pass reads the row of (step, slot[b])
    CondCall cc;
    std::vector<int64_t> distinct;
    std::vector<int> slots;
    if (c.labels) {
        SISIC_REQUIRE(std::isfinite(c.w), "sample_cond: guidance_scale %g", (double)c.w);
        cc.guided = c.w != 1.0f;
        cc.rows = cc.guided ? 2 * B : B;
        cc.w = c.w;
        SISIC_REQUIRE(cc.rows <= 65535, "sample_cond: batch %d", B);
        if (cc.guided)
            SISIC_REQUIRE(c.null_label >= 0 && c.null_label < u->n_class, "sample_cond: null_label %d is outside [0, %d)", c.null_label, u->n_class);
        auto slot_of = [&](int64_t label) -> int {
            const auto it = std::find(distinct.begin(), distinct.end(), label);
            if (it != distinct.end()) return (int)(it - distinct.begin());
            distinct.push_back(label);
            return (int)distinct.size() - 1;
        };
        slots.resize(cc.rows);
        for (int b = 0; b < B; ++b) slots[b] = slot_of(c.labels[b]);
        for (int b = B; b < cc.rows; ++b) slots[b] = slot_of(c.null_label);
        c.cg = &cc;
    }
    const bool guided = c.cg && c.cg->guided;
    const int rows = c.cg ? c.cg->rows : B;                      // samples per UNet pass
    const size_t L = c.cg ? distinct.size() : 1;                 // embedding rows per step
    SISIC_TRY(unet_check_shape(u, rows, H, W));
    // per-step tables for 1000 rows from the first call on (17 MB): a longer run after a shorter one then never moves the
    // time-embedding table, so the captured step (which holds its address) survives a change of T (and, in a conditional
    // call, a change of the labels as long as T x distinct labels stays within what the table has grown to)
    SISIC_TRY(unet_ensure_rows(u, std::max((size_t)T * L, (size_t)1000), (size_t)rows));
    const int C = u->cfg.in_channels;
    SISIC_REQUIRE(u->cfg.out_channels == C, "sample: in/out channels differ");
    const size_t n = (size_t)B * C * H * W;
    SISIC_TRY(unet_grow(&u->eps_buf, &u->eps_floats, (size_t)rows * C * H * W));
    if (c.rule == STEP_RULE_DPMPP) SISIC_TRY(unet_grow(&u->hist_buf, &u->hist_cap, n));
    // dynamic thresholding: every image's s of the step, [B] (a guided call steps B images)
    if (u->thr_ratio > 0.0f) {
        SISIC_REQUIRE((size_t)C * H * W <= ((size_t)1 << 24), "sample: thresholding takes images of at most 2^24 elements, these have %zu",
                      (size_t)C * H * W);
        SISIC_TRY(unet_grow(&u->thr_s, &u->thr_s_cap, (size_t)std::max(B, 64)));
    }
    if (c.cl) {
        // the loop's device table of the call: {scale, -, -, -, int target[B]} (elementwise.hip, LoopClf)
        std::vector<float> ct(LOOP_CLF_HEAD + (size_t)B, 0.0f);
        ct[0] = c.cl->scale;
        for (int b = 0; b < B; ++b) {
            const int t = (int)c.cl->targets[b];
            std::memcpy(&ct[LOOP_CLF_HEAD + b], &t, sizeof(int));
        }
        SISIC_TRY(unet_grow(&u->clf_tables, &u->clf_tables_cap, LOOP_CLF_HEAD + (size_t)std::max(B, 128)));
        SISIC_TRY(unet_stage_upload(u, ct.data(), ct.size(), u->clf_tables, s));
        SISIC_TRY(unet_grow(&u->clf_grad, &u->clf_grad_cap, n));
    }
    if (c.seeds) {
        // 2^31 step indices is ample (a run has at most 1000) and keeps step0 + i inside the int of the device-side state
        SISIC_REQUIRE(c.step0 >= 0 && c.step0 <= INT32_MAX - T, "sample_rng: step0 %d", c.step0);
        static_assert(sizeof(uint64_t) == 2 * sizeof(float), "seeds are staged as pairs of floats");
        SISIC_TRY(unet_grow(&u->seeds_dev, &u->seeds_cap, 2 * (size_t)std::max(B, 64)));
        SISIC_TRY(unet_stage_upload(u, reinterpret_cast<const float*>(c.seeds), 2 * (size_t)B, u->seeds_dev, s));
    }

    // every step's time embedding and time_emb_proj rows in one batch before the loop: row i of an unconditional call, row
    // i * L + j for slot j of a conditional one (linear_t computes each row on its own: a sample's embedding bits depend on its
    // (t, label) alone)
    std::vector<float> tv((size_t)T * L);
    for (size_t i = 0; i < (size_t)T; ++i)
        for (size_t j = 0; j < L; ++j) tv[i * L + j] = (float)c.timesteps[i];
    SISIC_TRY(unet_stage_upload(u, tv.data(), tv.size(), u->t_vals, s));
    if (c.cg) {
        std::vector<int64_t> lab((size_t)T * L);
        for (size_t i = 0; i < (size_t)T; ++i)
            for (size_t j = 0; j < L; ++j) lab[i * L + j] = distinct[j];
        SISIC_TRY(unet_upload_labels(u, lab.data(), (int)lab.size(), &u->labels_dev, &u->labels_cap, s));
        // the loop's device table of the call: {w, L, -, -, slot[rows]} (elementwise.hip, LoopCond)
        std::vector<float> ct(LOOP_COND_HEAD + (size_t)rows, 0.0f);
        const int Li = (int)L;
        ct[0] = c.cg->w;
        std::memcpy(&ct[1], &Li, sizeof(int));
        std::memcpy(&ct[LOOP_COND_HEAD], slots.data(), (size_t)rows * sizeof(int));
        SISIC_TRY(unet_grow(&u->cond_tables, &u->cond_tables_cap, LOOP_COND_HEAD + (size_t)std::max(rows, 128)));
        SISIC_TRY(unet_stage_upload(u, ct.data(), ct.size(), u->cond_tables, s));
    }
    SISIC_TRY(time_embed(u, (int)((size_t)T * L), s, c.cg != nullptr));

    // xs: the latent the steps run on, ls: their stream.  The replayed form steps the library's x_work, on a stream of the
    // library's own when the caller's is the legacy default stream; the eager form steps x in place on the caller's stream,
    // except that a guided call steps a library-owned [2B] copy (the step kernel writes both halves: the next pass reads them
    // without a copy).
    const bool use_graph = (u->graph_mode < 0 ? u->latency_mode : u->graph_mode != 0) && !u->ctx->profiling && T >= 4 && T <= 1000;
    float* xs = c.x;
    hipStream_t ls = s;
    if (use_graph) {
        if (!s) SISIC_HIP(hipStreamSynchronize(s));           // the embeddings above ran on the default stream
        SISIC_TRY(replay_begin(u, c, n, &ls));
        xs = u->x_work;
    } else {
        if (guided) {
            SISIC_TRY(unet_grow(&u->x_work, &u->x_work_cap, 2 * n));
            xs = u->x_work;
            SISIC_HIP(hipMemcpyAsync(xs, c.x, n * sizeof(float), hipMemcpyDeviceToDevice, s));
            SISIC_HIP(hipMemcpyAsync(xs + n, c.x, n * sizeof(float), hipMemcpyDeviceToDevice, s));
        }
        if (c.cg) SISIC_TRY(unet_grow(&u->tproj_cur, &u->tproj_cur_cap, (size_t)rows * u->tproj_R));
    }
    int i = 0;
    size_t zi = 0;                 // eager form: noise rows used so far
    bool ready = false;            // replayed form: the call has found or captured its graph
    auto steps = [&]() -> int {
        for (; i < T; ++i) {
            if (c.cancel) {
                if ((i & 7) == 0) SISIC_HIP(hipStreamSynchronize(ls));   // bound the run-ahead so a stop request takes effect
                if (*c.cancel) return SISIC_ECANCEL;
            }
            SISIC_TRY(use_graph ? replay_step(u, c, n, ls, i, &ready) : eager_step(u, c, xs, n, ls, i, &zi));
            const int row = c.traj_row ? c.traj_row[i] : i;          // (kept frames only: XAI.py:751-757 save_indices)
            if (c.traj && row >= 0) SISIC_HIP(hipMemcpyAsync(c.traj + (size_t)row * n, xs, n * sizeof(float), hipMemcpyDeviceToDevice, ls));
            if (c.steps_done) *c.steps_done = i + 1;
        }
        return SISIC_OK;
    };
    const int rc = steps();
    // x holds the latent after the steps that ran under every exit: a cancelled or failed run hands its partially stepped copy
    // back too
    if (xs != c.x) SISIC_HIP(hipMemcpyAsync(c.x, xs, n * sizeof(float), hipMemcpyDeviceToDevice, ls));
    if (ls != s) SISIC_HIP(hipStreamSynchronize(ls));         // hand the result back to the default stream's order
    if (rc == SISIC_ECANCEL) {
        SISIC_HIP(hipStreamSynchronize(ls));
        set_error("sample: cancelled after %d of %d steps", i, T);
    }
    if (rc != SISIC_OK) return rc;
    if (c.out_u8) SISIC_TRY(launch_denorm_u8(u->ctx, c.x, c.out_u8, B, C, H, W, s));
    return SISIC_OK;
}

int sisic_sample(sisic_unet* u, float* x, int B, int H, int W, int T, const int64_t* timesteps, const float* coef,
                 float clip, const float* noise, float* traj, uint8_t* out_u8, const volatile int* cancel,
                 int* steps_done, void* stream) {
    return sisic_sample_frames(u, x, B, H, W, T, timesteps, coef, clip, noise, traj, nullptr, out_u8, cancel, steps_done, stream);
}

// what every public entry point of the loop passes on as it was given; each adds its own fields
static LoopCall loop_call(float* x, int B, int H, int W, int T, const int64_t* timesteps, const float* coef, float clip, int rule,
                          int rule_flags, float* traj, const int* traj_row, uint8_t* out_u8, const volatile int* cancel,
                          int* steps_done, void* stream) {
    LoopCall c;
    c.x = x; c.B = B; c.H = H; c.W = W; c.T = T; c.timesteps = timesteps; c.coef = coef; c.clip = clip;
    c.rule = rule; c.rule_flags = rule_flags;
    c.traj = traj; c.traj_row = traj_row; c.out_u8 = out_u8; c.cancel = cancel; c.steps_done = steps_done; c.stream = stream;
    return c;
}

int sisic_sample_frames_rule(sisic_unet* u, float* x, int B, int H, int W, int T, const int64_t* timesteps, const float* coef,
                             float clip, int rule, int rule_flags, const float* noise, float* traj, const int* traj_row,
                             uint8_t* out_u8, const volatile int* cancel, int* steps_done, void* stream) {
    LoopCall c = loop_call(x, B, H, W, T, timesteps, coef, clip, rule, rule_flags, traj, traj_row, out_u8, cancel, steps_done, stream);
    c.noise = noise;
    return sample_frames(u, c);
}

int sisic_sample_frames_rule_rng(sisic_unet* u, float* x, int B, int H, int W, int T, const int64_t* timesteps,
                                 const float* coef, float clip, int rule, int rule_flags, const uint64_t* seeds, int step0,
                                 float* traj, const int* traj_row, uint8_t* out_u8, const volatile int* cancel, int* steps_done,
                                 void* stream) {
    SISIC_REQUIRE(seeds, "sample_rng: seeds is NULL");
    LoopCall c = loop_call(x, B, H, W, T, timesteps, coef, clip, rule, rule_flags, traj, traj_row, out_u8, cancel, steps_done, stream);
    c.seeds = seeds; c.step0 = step0;
    return sample_frames(u, c);
}

int sisic_sample_frames_cond(sisic_unet* u, float* x, int B, int H, int W, int T, const int64_t* timesteps, const float* coef,
                             float clip, int rule, int rule_flags, const float* noise, const uint64_t* seeds, int step0,
                             const int64_t* class_labels, int null_label, float guidance_scale, float* traj, const int* traj_row,
                             uint8_t* out_u8, const volatile int* cancel, int* steps_done, void* stream) {
    SISIC_REQUIRE(u && class_labels, "sample_cond: null argument");
    SISIC_REQUIRE(!(seeds && noise), "sample_cond: a noise buffer and seeds (host noise takes seeds NULL, device noise takes noise NULL)");
    LoopCall c = loop_call(x, B, H, W, T, timesteps, coef, clip, rule, rule_flags, traj, traj_row, out_u8, cancel, steps_done, stream);
    c.noise = noise; c.seeds = seeds; c.step0 = step0;
    c.labels = class_labels; c.null_label = null_label; c.w = guidance_scale;
    return sample_frames(u, c);
}

int sisic_sample_frames_edit(sisic_unet* u, float* x, int B, int H, int W, int T, const int64_t* timesteps, const float* coef,
                             float clip, int rule, int rule_flags, const uint64_t* seeds, int step0, const int64_t* class_labels,
                             int null_label, float guidance_scale, const float* x0k, const float* mask, const float* edit_rows,
                             float* traj, const int* traj_row, uint8_t* out_u8, const volatile int* cancel, int* steps_done,
                             void* stream) {
    SISIC_REQUIRE(u && seeds && x0k && mask && edit_rows,
                  "sample_edit: null argument (the known image, the mask, the edit rows and the seeds are required)");
    SISIC_REQUIRE(x0k != x && mask != x, "sample_edit: the known image or the mask is the latent buffer");
    const EditCall ed{x0k, mask, edit_rows};
    LoopCall c = loop_call(x, B, H, W, T, timesteps, coef, clip, rule, rule_flags, traj, traj_row, out_u8, cancel, steps_done, stream);
    c.seeds = seeds; c.step0 = step0;
    c.labels = class_labels; c.null_label = null_label; c.w = guidance_scale;
    c.ed = &ed;
    return sample_frames(u, c);
}

int sisic_guide_eps(sisic_ctx* ctx, const float* eps_c, const float* eps_u, float w, float* out, int64_t n, void* stream) {
    SISIC_REQUIRE(ctx, "guide_eps: null context");
    return launch_guide_eps(ctx, eps_c, eps_u, w, out, n, static_cast<hipStream_t>(stream));
}

int sisic_clf_guide_eps(sisic_ctx* ctx, sisic_clf_guide_args* a) {
    SISIC_REQUIRE(ctx && a, "clf_guide_eps: null argument");
    return launch_clf_guide_eps(ctx, a->eps, a->g, a->sb, a->scale, a->out, a->n, static_cast<hipStream_t>(a->stream));
}

// every refusal before the first launch; then sample_frames' loop with the classifier in it
int sisic_sample_frames_clf(sisic_unet* u, sisic_sample_clf_args* a) {
    SISIC_REQUIRE(u && a, "sample_clf: null argument");
    a->steps_done = 0;
    SISIC_REQUIRE(a->x && a->timesteps && a->coef && a->classifier && a->targets && a->B > 0 && a->T > 0, "sample_clf: null argument");
    SISIC_REQUIRE(u->n_class == 0, "sample_clf: a class-conditional handle (classifier guidance steers an unconditional model; "
                  "classifier-free guidance is sisic_sample_frames_cond)");
    SISIC_REQUIRE(u->pred_type == SISIC_PRED_EPSILON, "sample_clf: the handle's prediction_type is %d: classifier guidance takes "
                  "epsilon-prediction models only", u->pred_type);
    SISIC_REQUIRE(!a->noise && a->seeds, "sample_clf: host noise (a noise buffer, or no seeds): classifier guidance draws its noise "
                  "on the device");
    SISIC_REQUIRE(resnet_ctx(a->classifier) == u->ctx, "sample_clf: the classifier belongs to another context or device");
    SISIC_REQUIRE(resnet_loaded(a->classifier), "sample_clf: the classifier is not loaded (sisic_resnet_load)");
    SISIC_REQUIRE(a->H > 0 && a->W > 0 && a->H <= 224 && a->W <= 224, "sample_clf: latent %dx%d larger than the classifier's 224x224",
                  a->H, a->W);
    const int nc = resnet_num_classes(a->classifier);
    for (int b = 0; b < a->B; ++b)
        SISIC_REQUIRE(a->targets[b] >= 0 && a->targets[b] < nc, "sample_clf: target %lld of image %d is outside [0, %d)",
                      (long long)a->targets[b], b, nc);
    SISIC_REQUIRE(std::isfinite(a->scale), "sample_clf: classifier scale %g", (double)a->scale);
    SISIC_REQUIRE(u->cfg.in_channels == 3, "sample_clf: the classifier reads 3-channel images, the model has %d", u->cfg.in_channels);
    const ClfCall cl{a->classifier, a->targets, a->scale};
    LoopCall c = loop_call(a->x, a->B, a->H, a->W, a->T, a->timesteps, a->coef, a->clip, a->rule, a->rule_flags, a->traj, a->traj_row,
                           a->out_u8, a->cancel, &a->steps_done, a->stream);
    c.seeds = a->seeds; c.step0 = a->step0;
    c.cl = &cl;
    return sample_frames(u, c);
}

int sisic_sample_frames(sisic_unet* u, float* x, int B, int H, int W, int T, const int64_t* timesteps, const float* coef,
                        float clip, const float* noise, float* traj, const int* traj_row, uint8_t* out_u8,
                        const volatile int* cancel, int* steps_done, void* stream) {
    return sisic_sample_frames_rule(u, x, B, H, W, T, timesteps, coef, clip, SISIC_RULE_DDPM, 0, noise, traj, traj_row, out_u8,
                                    cancel, steps_done, stream);
}

int sisic_sample_frames_rng(sisic_unet* u, float* x, int B, int H, int W, int T, const int64_t* timesteps, const float* coef,
                            float clip, const uint64_t* seeds, int step0, float* traj, const int* traj_row, uint8_t* out_u8,
                            const volatile int* cancel, int* steps_done, void* stream) {
    return sisic_sample_frames_rule_rng(u, x, B, H, W, T, timesteps, coef, clip, SISIC_RULE_DDPM, 0, seeds, step0, traj,
                                        traj_row, out_u8, cancel, steps_done, stream);
}

}  // extern "C"
