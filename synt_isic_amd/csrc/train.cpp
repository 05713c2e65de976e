// train.cpp -- one UNet training step on the HIP kernels.
//
// Mirrors the loop body of diffusion/train_diffusion.py:211-240
//     noisy = scheduler.add_noise(images, noise, timesteps)            sisic_add_noise
//     noise_pred = model(noisy, timesteps).sample                      sisic_unet_train_forward  (records a tape)
//     loss = F.mse_loss(noise_pred, noise)                             sisic_mse_loss            (loss and d loss / d pred)
//     scaler.scale(loss).backward()                                    sisic_unet_backward       (walks the tape backwards)
//     scaler.step(optimizer); scaler.update()                          sisic_unet_optimizer_step (unscale, inf check, Adam)
// and sisic_unet_train_step runs the five in one call on one stream.  One path: the three fused steps (plain, _ext, _cond) fill
// the arguments of one train_step; every optimizer step, the classifier's included, is adam_step (train.h: a statistics pass
// when clipping, the norm or found_inf is asked for, then one fused Adam + EMA pass); every loss is one kernel
// (mse_objective_kernel); every job table goes up through upload_pack_table.  The training kernels have no atomics at all.
// The forward is the inference executor of unet.cpp in tape mode: same kernels (Winograd / direct MFMA convolutions with fused GroupNorm+SiLU prologues, GroupNorm
// statistics from convolution epilogues, attention), nothing released, every GroupNorm's scale/shift/(mean, rstd) kept.
// Backward per convolution: bias / time-embedding sums, backward-weight (conv_wgrad_kernel), backward-data as a
// forward convolution with transposed filters, then GroupNorm+SiLU backward into the input's gradient.
// Parity-test surface: sisic_unet_read copies a tensor's parameter / gradient / Adam moments to the host, sisic_unet_write
// puts a gradient or a moment of the caller's choosing into the arena (tests/test_gpu_optimizer.py).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>

#include "conv_plan.h"
#include "train.h"
#include "unet_internal.h"

using namespace sisic;

int sisic::upload_pack_table(std::vector<PackJob>& jobs, void** dev, int* njobs, int* nblocks) {
    int blocks = 0;
    for (PackJob& j : jobs) { j.first_block = blocks; blocks += pack_job_blocks(j); }
    if (*dev) { (void)hipFree(*dev); *dev = nullptr; }
    const size_t bytes = std::max<size_t>(jobs.size(), 1) * sizeof(PackJob);         // (an empty table still has an address)
    SISIC_HIP(hipMalloc(dev, bytes));
    SISIC_TRY(poison_fresh(*dev, bytes));
    if (!jobs.empty()) SISIC_HIP(hipMemcpy(*dev, jobs.data(), jobs.size() * sizeof(PackJob), hipMemcpyHostToDevice));
    *njobs = (int)jobs.size();
    *nblocks = blocks;
    return SISIC_OK;
}

// what TrainState owns on the device (the tape's pool blocks are the handle's: unet_release_tape)
TrainState::~TrainState() {
    for (void* p : {(void*)grad, (void*)adam_m, (void*)adam_v, (void*)emb, (void*)h1, (void*)t2, (void*)dtproj, (void*)labels_dev,
                    (void*)garena, (void*)wgrad_part, (void*)scratch, (void*)small, (void*)loss_dev, (void*)mse_part, stats_dev,
                    (void*)ema, repack_dev[0], repack_dev[1], repack_dev[2], scatter_dev})
        if (p) (void)hipFree(p);
}

namespace {

float* grad_of(sisic_unet* u, int idx) { return u->train->grad + u->offsets[idx]; }

// filters of the backward-data convolutions, rebuilt from the raw arena (after load and after every optimizer step)
int prepare_backward_conv(sisic_unet* u, ConvW& c, hipStream_t s) {
    if (c.k == 0) return SISIC_OK;
    const int kk = c.k * c.k;
    SISIC_TRY(dev_alloc(u->owned, (size_t)c.cout * c.cin * kk, &c.raw_t));
    SISIC_TRY(launch_transpose_flip(u->ctx, u->rawp(c.w_idx), c.cout, c.cin, kk, c.raw_t, s));
    SISIC_TRY(dev_alloc(u->owned, (size_t)sisic_conv_packed_numel(c.cin, c.cout, c.k), &c.packed_t));
    SISIC_TRY(launch_conv_pack(u->ctx, c.raw_t, c.cin, c.cout, c.k, c.packed_t, s));
    if (c.k == 3 && !c.strided && c.cin > 4) {
        SISIC_TRY(dev_alloc(u->owned, (size_t)winograd_packed_numel(c.cin, c.cout), &c.wino_t));
        SISIC_TRY(launch_winograd_pack(u->ctx, c.raw_t, c.cin, c.cout, c.wino_t, s));
    }
    return SISIC_OK;
}

// The job tables of repack.hip: everything unet_prepare_all (unet.cpp) and prepare_backward_weights (below) derive from the raw
// arena, in dependency order.  Built after those two have run once (they allocate); the destinations do not move afterwards.
int build_repack_plan(sisic_unet* u) {
    TrainState* tr = u->train.get();
    std::vector<PackJob> ph[3];
    const int nin = 2 * u->cfg.n_freqs;
    ph[0].push_back(pack_job_transpose2d(u->rawp(u->temb_w1), u->hidden, nin, u->w1t, u->hidden, 0));
    ph[0].push_back(pack_job_transpose2d(u->rawp(u->temb_w2), u->hidden, u->hidden, u->w2t, u->hidden, 0));
    for (ConvW* c : unet_convs(u)) {
        if (c->k == 0) continue;
        const float* w = u->rawp(c->w_idx);
        SISIC_REQUIRE(c->packed, "repack plan: forward filters are not prepared");
        ph[0].push_back(pack_job_conv(w, c->cout, c->cin, c->k, c->packed));
        if (c->wino) {
            ph[0].push_back(pack_job_wino_first(w, c->cout, c->cin, c->wino));
            ph[1].push_back(pack_job_wino_wide(c->cout, c->cin, c->wino));
            ph[1].push_back(pack_job_wino_bf3(c->cout, c->cin, c->wino));
        }
        if (c->s2) ph[0].push_back(pack_job_conv_s2(w, c->cout, c->cin, c->s2));
        if (c == &u->conv_in) continue;                       // the network input needs no gradient
        SISIC_REQUIRE(c->raw_t && c->packed_t, "repack plan: backward filters are not prepared");
        ph[0].push_back(pack_job_flip(w, c->cout, c->cin, c->k * c->k, c->raw_t));
        ph[1].push_back(pack_job_conv(c->raw_t, c->cin, c->cout, c->k, c->packed_t));
        if (c->wino_t) {
            ph[1].push_back(pack_job_wino_first(c->raw_t, c->cin, c->cout, c->wino_t));
            ph[2].push_back(pack_job_wino_wide(c->cin, c->cout, c->wino_t));
            ph[2].push_back(pack_job_wino_bf3(c->cin, c->cout, c->wino_t));
        }
    }
    for (ResnetW* r : unet_resnets(u)) {
        ph[0].push_back(pack_job_transpose2d(u->rawp(r->temb_w_idx), r->cout, u->hidden, u->tproj_wt, u->tproj_R, r->temb_off));
        ph[0].push_back(pack_job_copy(u->rawp(r->temb_b_idx), u->tproj_b + r->temb_off, (size_t)r->cout));
    }
    for (AttnW* a : unet_attns(u)) {
        const int c = a->c;
        SISIC_REQUIRE(a->qkv_cat && a->qkv_packed && a->qkv_bias && a->qkv_raw_t && a->qkv_packed_t, "repack plan: attention filters are not prepared");
        const int wi[3] = {a->q_w, a->k_w, a->v_w}, bi[3] = {a->q_b, a->k_b, a->v_b};
        for (int i = 0; i < 3; ++i) {
            ph[0].push_back(pack_job_copy(u->rawp(wi[i]), a->qkv_cat + (size_t)i * c * c, (size_t)c * c));
            ph[0].push_back(pack_job_copy(u->rawp(bi[i]), a->qkv_bias + (size_t)i * c, (size_t)c));
        }
        ph[1].push_back(pack_job_conv(a->qkv_cat, 3 * c, c, 1, a->qkv_packed));
        ph[1].push_back(pack_job_flip(a->qkv_cat, 3 * c, c, 1, a->qkv_raw_t));
        ph[2].push_back(pack_job_conv(a->qkv_raw_t, c, 3 * c, 1, a->qkv_packed_t));
    }
    for (int p = 0; p < 3; ++p) SISIC_TRY(upload_pack_table(ph[p], &tr->repack_dev[p], &tr->repack_jobs[p], &tr->repack_blocks[p]));
    tr->repack_ready = true;
    return SISIC_OK;
}

int run_repack_plan(sisic_unet* u, hipStream_t s) {
    TrainState* tr = u->train.get();
    for (int p = 0; p < 3; ++p)
        SISIC_TRY(launch_pack_batch(u->ctx, static_cast<const PackJob*>(tr->repack_dev[p]), tr->repack_jobs[p], tr->repack_blocks[p], s));
    return SISIC_OK;
}

int prepare_backward_weights(sisic_unet* u, hipStream_t s) {
    for (ConvW* c : unet_convs(u))
        if (c != &u->conv_in) SISIC_TRY(prepare_backward_conv(u, *c, s));     // the network input needs no gradient
    for (AttnW* a : unet_attns(u)) {
        const int c = a->c;
        SISIC_TRY(dev_alloc(u->owned, (size_t)3 * c * c, &a->qkv_raw_t));
        SISIC_TRY(launch_transpose_flip(u->ctx, a->qkv_cat, 3 * c, c, 1, a->qkv_raw_t, s));
        SISIC_TRY(dev_alloc(u->owned, (size_t)sisic_conv_packed_numel(c, 3 * c, 1), &a->qkv_packed_t));
        SISIC_TRY(launch_conv_pack(u->ctx, a->qkv_raw_t, c, 3 * c, 1, a->qkv_packed_t, s));
    }
    return SISIC_OK;
}

struct Bwd {
    sisic_unet* u;
    TrainState* tr;
    hipStream_t s;
    int B;

    static size_t arena_floats(size_t n) { return (n + 63) & ~size_t(63); }       // 256-byte aligned carve-outs

    // gradient buffer of an activation: carved from the arena that run() zero-filled in one go (one fill instead of one
    // per activation: 85 launches of ~6 us at batch 32)
    int grad(Buf* b, float** out) {
        auto it = tr->buf_grad.find(b);
        if (it != tr->buf_grad.end()) { *out = it->second; return SISIC_OK; }
        const size_t n = arena_floats((size_t)B * b->C * b->H * b->W);
        SISIC_REQUIRE(tr->garena_used + n <= tr->garena_cap, "backward: gradient arena exhausted");
        float* g = tr->garena + tr->garena_used;
        tr->garena_used += n;
        tr->buf_grad[b] = g;
        *out = g;
        return SISIC_OK;
    }

    int conv_op(const TapeOp& op, const float* dout) {
        const ConvW& c = op.w;
        const int Cin = op.c0 + op.c1;
        const int Hc = op.H << (op.ups ? 1 : 0), Wc = op.W << (op.ups ? 1 : 0);
        const int pad = c.k / 2;
        const int Ho = (Hc + 2 * pad - c.k) / op.stride + 1, Wo = (Wc + 2 * pad - c.k) / op.stride + 1;
        const float* dy = dout;
        if (op.out) {
            float* g = nullptr;
            SISIC_TRY(grad(op.out, &g));
            dy = g;
        }
        SISIC_REQUIRE(dy, "backward: no gradient for the network output");
        // ---- residual input: the gradient passes through unchanged
        if (op.residual) {
            float* gr = nullptr;
            SISIC_TRY(grad(op.residual, &gr));
            SISIC_TRY(launch_add_inplace(u->ctx, gr, dy, (size_t)B * c.cout * Ho * Wo, s));
        }
        // ---- bias and time-embedding projection: sums of dy over the pixels of each (sample, channel) plane, one launch
        if (op.qkv_of) {
            SISIC_TRY(launch_bias_grad(u->ctx, dy, B, c.cout, Ho * Wo, grad_of(u, op.qkv_of->q_b), grad_of(u, op.qkv_of->k_b),
                                       grad_of(u, op.qkv_of->v_b), op.qkv_of->c, nullptr, 0, s));
        } else {
            SISIC_TRY(launch_bias_grad(u->ctx, dy, B, c.cout, Ho * Wo, grad_of(u, c.b_idx), nullptr, nullptr, 0,
                                       op.temb_off >= 0 ? tr->dtproj + op.temb_off : nullptr, u->tproj_R, s));
        }
        // ---- weights
        {
            WgradArgs a;
            a.in0 = op.in0_ptr; a.in1 = op.in1_ptr; a.c0 = op.c0; a.c1 = op.c1; a.B = B; a.Hin = op.H; a.Win = op.W;
            a.ups = op.ups; a.ksize = c.k; a.stride = op.stride;
            a.gn_scale = op.gn_scale; a.gn_shift = op.gn_shift; a.gn_silu = op.silu ? 1 : 0;
            a.dy = dy; a.Cout = c.cout;
            const size_t need = conv_wgrad_scratch_floats(a);
            SISIC_TRY(unet_grow(&tr->wgrad_part, &tr->wgrad_part_cap, need));
            if (op.qkv_of) {            // [3C, C] leaves the reduction as the three projections' gradients
                a.dw = grad_of(u, op.qkv_of->q_w); a.dw1 = grad_of(u, op.qkv_of->k_w); a.dw2 = grad_of(u, op.qkv_of->v_w);
            } else {
                a.dw = grad_of(u, c.w_idx);
            }
            SISIC_TRY(launch_conv_wgrad(u->ctx, a, tr->wgrad_part, need, s));
        }
        // ---- data
        if (!op.in0) return SISIC_OK;                          // the network input
        const float* packed_t = op.qkv_of ? op.qkv_of->qkv_packed_t : c.packed_t;
        SISIC_REQUIRE(packed_t, "backward: the backward-data filters have not been prepared");
        const size_t da_n = (size_t)B * Cin * Hc * Wc;
        SISIC_TRY(unet_grow(&tr->scratch, &tr->scratch_cap, da_n));
        float* da = tr->scratch;
        float* g0 = nullptr;
        float* g1 = nullptr;
        SISIC_TRY(grad(op.in0, &g0));
        if (op.in1) SISIC_TRY(grad(op.in1, &g1));
        // an input that is neither normalised, nor upsampled, nor a concatenation receives its gradient straight from the
        // convolution's epilogue: out = conv(dy) + residual with residual = out = the input's gradient buffer (every element is
        // read and then written by the same thread) -- no scratch tensor, no accumulate launch; g + y in place of g += y: same bits
        const bool in_place = !op.norm && !op.ups && !op.in1;
        {
            sisic_conv_args a{};
            a.in0 = dy; a.c0 = c.cout; a.B = B; a.Hin = Ho; a.Win = Wo;
            a.ksize = c.k; a.stride = 1; a.upsample = op.stride == 2 ? 2 : 0;
            a.w_packed = packed_t; a.Cout = Cin;
            a.w_winograd = (op.stride == 1 && !op.qkv_of && u->use_winograd) ? c.wino_t : nullptr;
            a.out = da;
            if (in_place) { a.out = g0; a.residual = g0; }
            if (u->latency_mode) a.tile_cfg = conv_latency_cfg(a);      // the forward's small-batch tile choices for the data gradient
            SISIC_TRY(launch_conv2d(u->ctx, a, s));
        }
        if (in_place) return SISIC_OK;
        if (op.norm) {
            float* sums = tr->small + (size_t)B * c.cout;      // [2][B][Cin]
            SISIC_TRY(launch_gn_bwd(u->ctx, da, op.in0_ptr, op.c0, op.in1_ptr, op.c1, B, op.H * op.W, u->cfg.norm_groups,
                                    op.gn_scale, op.gn_shift, op.gn_mr, op.norm->gamma, op.silu ? 1 : 0, sums, g0, g1,
                                    grad_of(u, op.norm->w_idx), grad_of(u, op.norm->b_idx), s));
        } else if (op.ups) {
            SISIC_TRY(launch_accum_pool2(u->ctx, da, B * Cin, op.H, op.W, g0, s));
        } else {
            SISIC_TRY(launch_accum_split(u->ctx, da, B, Cin, op.H * op.W, g0, op.c0, g1, op.c1, s));
        }
        return SISIC_OK;
    }

    int attn_op(const TapeOp& op) {
        float* dO = nullptr;
        float* dqkv = nullptr;
        SISIC_TRY(grad(op.o, &dO));
        SISIC_TRY(grad(op.qkv, &dqkv));                        // zero-filled; the kernel overwrites every element
        return launch_attention_bwd(u->ctx, op.qkv->p, op.o->p, dO, dqkv, B, op.C, op.N, u->cfg.head_dim, s);
    }

    // hd = dropout(silu(norm2(h))): conv2's backward-data has left d hd in hd's gradient buffer (its in-place form); the mask,
    // regenerated, is applied there in one pass; the GroupNorm+SiLU backward that every normalised input takes runs on the result
    int dropout_op(const TapeOp& op) {
        float* dhd = nullptr;
        float* g0 = nullptr;
        SISIC_TRY(grad(op.out, &dhd));
        SISIC_TRY(grad(op.in0, &g0));
        const int C = op.c0, HW = op.H * op.W;
        SISIC_TRY(launch_dropout_bwd(u->ctx, dhd, B, C, HW, tr->drop_seed, tr->drop_call, 256u + (uint32_t)op.drop_block, tr->drop_p,
                                     tr->drop_inv_keep, s));
        float* sums = tr->small + (size_t)B * C;           // [2][B][C]
        return launch_gn_bwd(u->ctx, dhd, op.in0_ptr, C, nullptr, 0, B, HW, u->cfg.norm_groups, op.gn_scale, op.gn_shift, op.gn_mr,
                             op.norm->gamma, 1, sums, g0, nullptr, grad_of(u, op.norm->w_idx), grad_of(u, op.norm->b_idx), s);
    }

    // time embedding: tproj = time_emb_proj(ta), ta = silu(t2), t2 = linear_2(silu(h1)), h1 = linear_1(emb)
    int time_embedding() {
        const int R = u->tproj_R, Hd = u->hidden, nin = 2 * u->cfg.n_freqs;
        const size_t need = (size_t)R * Hd + R + (size_t)5 * B * Hd;
        SISIC_TRY(unet_grow(&tr->wgrad_part, &tr->wgrad_part_cap, need));
        float* dWf = tr->wgrad_part;                // [R][Hd]
        float* dbf = dWf + (size_t)R * Hd;          // [R]
        float* dta = dbf + R;                       // [B][Hd]
        float* dt2 = dta + (size_t)B * Hd;
        float* a1 = dt2 + (size_t)B * Hd;
        float* da1 = a1 + (size_t)B * Hd;
        float* dh1 = da1 + (size_t)B * Hd;
        // fused projection of the 22 residual blocks
        SISIC_TRY(launch_linear_wgrad(u->ctx, tr->dtproj, R, u->temb_act, B, R, Hd, dWf, s));
        SISIC_TRY(launch_col_sums(u->ctx, tr->dtproj, B, R, R, dbf, 0, s));
        // the 22 blocks' slices of the fused gradient to their own tensors: ONE launch over a job table (44 device copies before)
        if (!tr->scatter_dev || tr->scatter_src != dWf) {
            std::vector<PackJob> jobs;
            for (ResnetW* r : unet_resnets(u)) {
                jobs.push_back(pack_job_copy(dWf + (size_t)r->temb_off * Hd, grad_of(u, r->temb_w_idx), (size_t)r->cout * Hd));
                jobs.push_back(pack_job_copy(dbf + r->temb_off, grad_of(u, r->temb_b_idx), (size_t)r->cout));
            }
            SISIC_HIP(hipStreamSynchronize(s));          // (a table in use is not replaced under a running launch)
            SISIC_TRY(upload_pack_table(jobs, &tr->scatter_dev, &tr->scatter_jobs, &tr->scatter_blocks));
            tr->scatter_src = dWf;
        }
        SISIC_TRY(launch_pack_batch(u->ctx, static_cast<const PackJob*>(tr->scatter_dev), tr->scatter_jobs, tr->scatter_blocks, s));
        // d ta[b][k] = sum_r dtproj[b][r] * Wfused[r][k]; the fused weight is stored transposed: tproj_wt[k][r]
        SISIC_TRY(launch_linear_dgrad(u->ctx, tr->dtproj, R, u->tproj_wt, B, R, Hd, dta, s, /*w_is_transposed=*/1));
        SISIC_TRY(launch_silu_bwd(u->ctx, dta, tr->t2, (size_t)B * Hd, dt2, s));
        // class embedding: t2 = linear_2(a1) + E[label], so row k of dE is the sum of dt2 over the samples labelled k
        if (tr->has_labels)
            SISIC_TRY(launch_class_embed_grad(u->ctx, dt2, reinterpret_cast<const int*>(tr->labels_dev), B, u->n_class, Hd,
                                              grad_of(u, u->class_w), s));
        // linear_2: t2 = a1 W2^T + b2, a1 = silu(h1)
        SISIC_TRY(launch_silu_fwd(u->ctx, tr->h1, (size_t)B * Hd, a1, s));
        SISIC_TRY(launch_linear_wgrad(u->ctx, dt2, Hd, a1, B, Hd, Hd, grad_of(u, u->temb_w2), s));
        SISIC_TRY(launch_col_sums(u->ctx, dt2, B, Hd, Hd, grad_of(u, u->temb_b2), 0, s));
        SISIC_TRY(launch_linear_dgrad(u->ctx, dt2, Hd, u->rawp(u->temb_w2), B, Hd, Hd, da1, s, 0));
        SISIC_TRY(launch_silu_bwd(u->ctx, da1, tr->h1, (size_t)B * Hd, dh1, s));
        // linear_1: h1 = emb W1^T + b1
        SISIC_TRY(launch_linear_wgrad(u->ctx, dh1, Hd, tr->emb, B, Hd, nin, grad_of(u, u->temb_w1), s));
        SISIC_TRY(launch_col_sums(u->ctx, dh1, B, Hd, Hd, grad_of(u, u->temb_b1), 0, s));
        return SISIC_OK;
    }

    int run(const float* dout) {
        SISIC_HIP(hipMemsetAsync(tr->dtproj, 0, (size_t)B * u->tproj_R * sizeof(float), s));
        size_t total = 0;                        // every activation of the tape may receive a gradient
        for (auto& b : tr->bufs) total += arena_floats((size_t)B * b->C * b->H * b->W);
        SISIC_TRY(unet_grow(&tr->garena, &tr->garena_cap, total));
        tr->garena_used = 0;
        SISIC_HIP(hipMemsetAsync(tr->garena, 0, total * sizeof(float), s));
        for (auto it = tr->tape.rbegin(); it != tr->tape.rend(); ++it) {
            if (it->kind == TapeOp::CONV) SISIC_TRY(conv_op(*it, dout));
            else if (it->kind == TapeOp::DROPOUT) SISIC_TRY(dropout_op(*it));
            else SISIC_TRY(attn_op(*it));
        }
        return time_embedding();
    }
};

int require_train(sisic_unet* u, const char* what) {
    SISIC_REQUIRE(u, "%s: null handle", what);
    if (!u->loaded || !u->train) {
        set_error("%s: call sisic_unet_load and sisic_unet_train_begin first", what);
        return SISIC_ESTATE;
    }
    return SISIC_OK;
}

// At head_dim 8 the backward pass keeps an attention block's whole key/value rows in LDS (launch_attention_bwd); at 32 and 64 it
// is tiled and bounded by ATTN_BWD_TILED_MAX_TOKENS (train.h).  A resolution whose attention levels have more tokens than the
// model's head dimension takes records a forward that could never be back-propagated.  Refused before anything is recorded, so
// that no backward pass half-accumulates gradients before it fails.
int check_trainable_resolution(sisic_unet* u, int H, int W) {
    const sisic_unet_config& cfg = u->cfg;
    const int n = cfg.n_blocks;
    for (int lvl = 0; lvl < n; ++lvl) {
        // down block lvl, up block n-1-lvl and (at the lowest level) the mid block run at H >> lvl x W >> lvl
        if (!(cfg.down_attn[lvl] || cfg.up_attn[n - 1 - lvl] || lvl == n - 1)) continue;
        const int h = H >> lvl, w = W >> lvl;
        const int max_tokens = attn_bwd_max_tokens(cfg.head_dim);     // 1170 at head_dim 8 (LDS), 65536 at 32 and 64 (tiled)
        SISIC_REQUIRE((int64_t)h * w <= max_tokens,
                      "train_forward: %dx%d cannot be trained: its %dx%d attention level has %lld tokens, the attention backward "
                      "pass takes at most %d", H, W, h, w, (long long)h * w, max_tokens);
    }
    return SISIC_OK;
}

// every derived form of the weights follows a change of the raw arena (an optimizer step, an EMA swap): three batched
// launches (repack.hip); the one-launch-per-tensor route of the load path when the buffers have moved since the job tables
// were built (SISIC_REPACK_BATCH=0: always)
int repack_after_update(sisic_unet* u, hipStream_t s) {
    TrainState* tr = u->train.get();
    static const bool batch_on = [] { const char* e = std::getenv("SISIC_REPACK_BATCH"); return !e || std::atoi(e) != 0; }();
    if (batch_on && tr->repack_ready) return run_repack_plan(u, s);
    SISIC_TRY(unet_prepare_all(u, s));
    SISIC_TRY(prepare_backward_weights(u, s));
    if (batch_on) {
        SISIC_HIP(hipStreamSynchronize(s));
        SISIC_TRY(build_repack_plan(u));
    }
    return SISIC_OK;
}

// training on the averaged weights is always a bug
int require_not_swapped(sisic_unet* u, const char* what) {
    if (u->train->ema_swapped) {
        set_error("%s: the EMA weights are swapped in (sisic_unet_ema_swap): swap the trained weights back first", what);
        return SISIC_ESTATE;
    }
    return SISIC_OK;
}

// The one loss launch: stages the rows the objective reads -- {sa, sb} of the v target (coef: host [2B], with noise; else
// nullptr), then the handle's loss weights when it has any -- into objective_dev and runs the one kernel.  B: the samples n is
// divided into (the caller has checked the weight table against it).
int mse_objective(sisic_unet* u, const float* pred, const float* target, const float* noise, const float* coef, int B, size_t n,
                  float grad_scale, float* loss_dev, float* dpred, hipStream_t s) {
    const bool weighted = !u->loss_w.empty();
    const float* rows = nullptr;
    if (noise || weighted) {
        std::vector<float> host;
        if (noise) host.assign(coef, coef + 2 * (size_t)B);
        if (weighted) host.insert(host.end(), u->loss_w.begin(), u->loss_w.end());
        SISIC_TRY(unet_grow(&u->objective_dev, &u->objective_cap, 3 * (size_t)B));
        SISIC_TRY(unet_stage_upload(u, host.data(), host.size(), u->objective_dev, s));
        rows = u->objective_dev;
    }
    const float* w = weighted ? rows + (noise ? 2 * (size_t)B : 0) : nullptr;
    return launch_mse_objective(u->ctx, pred, target, noise, noise ? rows : nullptr, noise ? rows + B : nullptr, w, B, n, grad_scale,
                                loss_dev, dpred, u->train->mse_part, 2048, s);
}

// the loop body of sisic_unet_train_step up to the optimizer step: add_noise, forward, MSE, backward, the loss read-back
// class_labels: host int64 [B] of a conditional model, or nullptr
int train_forward_impl(sisic_unet* u, const float* sample, const int64_t* timesteps, const int64_t* class_labels, float* out, int B,
                       int H, int W, void* stream);

int train_step_body(sisic_unet* u, const float* images, const float* noise, const int64_t* timesteps, const int64_t* class_labels,
                    const float* sqrt_alpha_prod, const float* sqrt_one_minus_alpha_prod, int B, int H, int W, float loss_scale,
                    float* loss_out, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    TrainState* tr = u->train.get();
    const int C = u->cfg.in_channels;
    // The fused step regresses the prediction on a tensor of the INPUT's shape (the noise, the image or v) and lays out
    // noisy | prediction | d prediction as three blocks of that size: a model whose output has another channel count (the
    // learned-variance layout, out = 2 in) would write its prediction over d prediction.  As the sampling loops: refused
    // before any buffer is grown or any launch made.  (The spelled-out loop takes such a model: its target has the output's shape.)
    SISIC_REQUIRE(u->cfg.out_channels == C,
                  "train_step: in/out channels differ: the model maps %d input channels to %d output channels, and the fused step's "
                  "target has the input's shape", C, u->cfg.out_channels);
    const size_t n = (size_t)B * C * H * W;
    // a table left from another batch size is an error, never a silently unweighted (or wrongly weighted) loss
    const bool weighted = !u->loss_w.empty();
    SISIC_REQUIRE(!weighted || (int)u->loss_w.size() == B,
                  "train_step: %d loss weights are set, the batch is %d (sisic_unet_set_loss_weights)", (int)u->loss_w.size(), B);
    SISIC_TRY(unet_grow(&u->eps_buf, &u->eps_floats, 3 * n));     // noisy | prediction | d prediction
    float* noisy = u->eps_buf;
    float* pred = noisy + n;
    float* dpred = pred + n;
    // coefficient rows: host -> device through the pinned ring (2B floats)
    SISIC_TRY(unet_ensure_rows(u, (size_t)B, (size_t)B));
    SISIC_TRY(unet_grow(&tr->small, &tr->small_cap, train_small_floats(u, B)));
    std::vector<float> coef(2 * (size_t)B);
    std::memcpy(coef.data(), sqrt_alpha_prod, B * sizeof(float));
    std::memcpy(coef.data() + B, sqrt_one_minus_alpha_prod, B * sizeof(float));
    SISIC_TRY(unet_stage_upload(u, coef.data(), 2 * (size_t)B, tr->small, s));
    SISIC_TRY(launch_add_noise(u->ctx, images, noise, tr->small, tr->small + B, noisy, B, (size_t)C * H * W, s));
    SISIC_TRY(train_forward_impl(u, noisy, timesteps, class_labels, pred, B, H, W, stream));
    // the objective: the target follows the handle's prediction type -- the noise, the image, or v formed
    // in the loss kernel's registers from the two rows above (no target tensor) -- and the handle's loss weights apply
    const bool v = u->pred_type == SISIC_PRED_V;
    SISIC_TRY(mse_objective(u, pred, u->pred_type == SISIC_PRED_EPSILON ? noise : images, v ? noise : nullptr, v ? coef.data() : nullptr,
                            B, n, loss_scale, tr->loss_dev, dpred, s));
    SISIC_TRY(sisic_unet_backward(u, dpred, stream));
    if (loss_out) {
        SISIC_HIP(hipMemcpyAsync(loss_out, tr->loss_dev, sizeof(float), hipMemcpyDeviceToHost, s));
        SISIC_HIP(hipStreamSynchronize(s));
    }
    return SISIC_OK;
}

int train_forward_impl(sisic_unet* u, const float* sample, const int64_t* timesteps, const int64_t* class_labels, float* out, int B,
                       int H, int W, void* stream) {
    hipStream_t s = static_cast<hipStream_t>(stream);
    TrainState* tr = u->train.get();
    unet_release_tape(u);                                  // a forward without a backward: drop the old tape
    SISIC_TRY(unet_check_shape(u, B, H, W));
    SISIC_TRY(check_trainable_resolution(u, H, W));
    SISIC_TRY(unet_ensure_rows(u, (size_t)B, (size_t)B));
    const int Hd = u->hidden, nin = 2 * u->cfg.n_freqs;
    SISIC_TRY(unet_grow(&tr->emb, &tr->emb_cap, (size_t)B * nin));
    SISIC_TRY(unet_grow(&tr->h1, &tr->h1_cap, (size_t)B * Hd));
    SISIC_TRY(unet_grow(&tr->t2, &tr->t2_cap, (size_t)B * Hd));
    SISIC_TRY(unet_grow(&tr->dtproj, &tr->dtproj_cap, (size_t)B * u->tproj_R));
    SISIC_TRY(unet_grow(&tr->small, &tr->small_cap, train_small_floats(u, B)));
    std::vector<float> tv(B);
    for (int b = 0; b < B; ++b) tv[b] = (float)timesteps[b];
    SISIC_TRY(unet_stage_upload(u, tv.data(), (size_t)B, u->t_vals, s));
    // the labels go on the tape: the backward pass sums the class embedding's gradient rows by them
    tr->has_labels = class_labels != nullptr;
    if (class_labels) SISIC_TRY(unet_upload_labels(u, class_labels, B, &tr->labels_dev, &tr->labels_cap, s));
    // per-sample rows always (the training timesteps differ per image, train_diffusion.py:216), intermediates kept
    SISIC_TRY(launch_temb_mlp(u->ctx, u->t_vals, B, u->d_freqs, u->cfg.n_freqs, u->w1t, u->rawp(u->temb_b1), u->w2t,
                              u->rawp(u->temb_b2), Hd, u->temb_act, s, tr->emb, tr->h1, tr->t2,
                              class_labels ? u->rawp(u->class_w) : nullptr,
                              class_labels ? reinterpret_cast<const int*>(tr->labels_dev) : nullptr));
    SISIC_TRY(launch_linear_t(u->ctx, u->temb_act, B, Hd, u->tproj_wt, u->tproj_b, u->tproj_R, u->tproj, s));
    tr->B = B; tr->H = H; tr->W = W;
    // the dropout of this tape: the handle's setting and counter as they stand now (include/sisic.h, the mask contract)
    tr->drop_p = u->drop_p; tr->drop_seed = u->drop_seed; tr->drop_call = u->drop_call;
    tr->drop_inv_keep = (float)(1.0 / (1.0 - (double)u->drop_p));
    const int rc = unet_run_forward(u, sample, u->tproj, u->tproj_R, out, B, H, W, s, tr);
    if (rc != SISIC_OK) {
        unet_release_tape(u);
        return rc;
    }
    if (tr->drop_p > 0.0f) u->drop_call += 1;
    tr->has_tape = true;
    return SISIC_OK;
}

GradStats* stats_record(TrainState* tr) { return static_cast<GradStats*>(tr->stats_dev); }
void* stats_scratch(TrainState* tr) { return static_cast<char*>(tr->stats_dev) + 16; }

// The optimizer step of the three entry points that take one.  ext_entry: the call came through an _ext entry point (its
// statistics pass always runs, and grad_norm_out is written); otherwise the pass runs only for found_inf.
int optimizer_step(sisic_unet* u, const char* who, bool ext_entry, double lr, double beta1, double beta2, double eps, float inv_scale,
                   const sisic_optim_ext* ext, int* found_inf, float* grad_norm_out, hipStream_t s) {
    SISIC_TRY(require_train(u, who));
    SISIC_TRY(require_not_swapped(u, who));
    TrainState* tr = u->train.get();
    SISIC_HIP(hipSetDevice(u->ctx->device));
    const bool ema_on = ext && ext->ema_update != 0;
    if (ema_on) {
        if (!tr->ema) {
            set_error("%s: ema_update without an EMA arena (call sisic_unet_ema_begin first)", who);
            return SISIC_ESTATE;
        }
        SISIC_REQUIRE(ext->ema_decay >= 0.0 && ext->ema_decay <= 1.0, "%s: ema_decay %g is outside [0, 1]", who, ext->ema_decay);
    }
    AdamStepArgs a;
    a.p = u->raw; a.g = tr->grad; a.m = tr->adam_m; a.v = tr->adam_v; a.n = u->raw_floats;
    a.ema = ema_on ? tr->ema : nullptr; a.ema_decay = ema_on ? ext->ema_decay : 0.0;
    a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps;
    a.inv_scale = inv_scale; a.max_norm = ext ? ext->max_grad_norm : 0.0f;
    a.step = &tr->step; a.stats = stats_record(tr); a.scratch = stats_scratch(tr);
    a.want_stats = ext_entry || found_inf;       // GradScaler.step: without found_inf there is no check and no skip
    a.skip_on_inf = found_inf != nullptr;
    AdamStepResult r;
    SISIC_TRY(adam_step(u->ctx, a, &r, s));
    if (ext_entry && grad_norm_out) *grad_norm_out = r.norm;
    if (found_inf) *found_inf = r.found_inf;
    return r.skipped ? SISIC_OK : repack_after_update(u, s);
}

// The fused step of the three entry points: the checks, the loop body, the optimizer step.  `who` names the entry point in
// every refusal; cond: the entry takes labels; ext_entry: as optimizer_step.
struct TrainStepArgs {
    const char* who;
    bool cond, ext_entry;
    const float* images; const float* noise; const int64_t* timesteps; const int64_t* class_labels;
    const float* sqrt_alpha_prod; const float* sqrt_one_minus_alpha_prod;
    int B, H, W;
    double lr, beta1, beta2, eps;
    float loss_scale;
    const sisic_optim_ext* ext;
    float* loss_out; int* found_inf; float* grad_norm_out;
    void* stream;
};

int train_step(sisic_unet* u, const TrainStepArgs& a) {
    SISIC_TRY(require_train(u, a.who));
    SISIC_TRY(require_not_swapped(u, a.who));
    SISIC_REQUIRE(a.images && a.noise && a.timesteps && a.sqrt_alpha_prod && a.sqrt_one_minus_alpha_prod, "%s: null argument", a.who);
    SISIC_TRY(unet_check_labels(u, a.who, a.cond, a.class_labels, a.B));
    SISIC_TRY(train_step_body(u, a.images, a.noise, a.timesteps, a.class_labels, a.sqrt_alpha_prod, a.sqrt_one_minus_alpha_prod, a.B, a.H,
                              a.W, a.loss_scale, a.loss_out, a.stream));
    return optimizer_step(u, a.ext_entry ? "optimizer_step_ext" : "optimizer_step", a.ext_entry, a.lr, a.beta1, a.beta2, a.eps,
                          1.0f / a.loss_scale, a.ext, a.found_inf, a.grad_norm_out, static_cast<hipStream_t>(a.stream));
}

int train_forward(sisic_unet* u, const char* who, bool cond, const float* sample, const int64_t* timesteps, const int64_t* class_labels,
                  float* out, int B, int H, int W, void* stream) {
    SISIC_TRY(require_train(u, who));
    SISIC_REQUIRE(sample && timesteps && out, "%s: null argument", who);
    SISIC_TRY(unet_check_labels(u, who, cond, class_labels, B));
    return train_forward_impl(u, sample, timesteps, class_labels, out, B, H, W, stream);
}

}  // namespace

extern "C" {

int sisic_unet_train_begin(sisic_unet* u) {
    SISIC_REQUIRE(u, "train_begin: null handle");
    if (!u->loaded) {
        set_error("train_begin: load the weights first");
        return SISIC_ESTATE;
    }
    SISIC_HIP(hipSetDevice(u->ctx->device));
    if (!u->train) {
        auto tr = std::make_unique<TrainState>();
        // (a failure below frees what has been allocated: ~TrainState)
        auto alloc = [](size_t bytes, auto** out) {
            void* q = nullptr;
            SISIC_HIP(hipMalloc(&q, bytes));
            *out = static_cast<std::remove_reference_t<decltype(*out)>>(q);
            return poison_fresh(q, bytes);
        };
        for (float** p : {&tr->grad, &tr->adam_m, &tr->adam_v})
            SISIC_TRY(alloc(u->raw_floats * sizeof(float), p));            // (all three are zero-filled below, as ever)
        SISIC_TRY(alloc(4 * sizeof(float), &tr->loss_dev));
        SISIC_TRY(alloc(2048 * sizeof(float), &tr->mse_part));
        SISIC_TRY(alloc(16 + grad_stats_scratch_bytes(), &tr->stats_dev));
        u->train = std::move(tr);
    }
    TrainState* tr = u->train.get();
    SISIC_TRY(require_not_swapped(u, "train_begin"));
    const size_t bytes = u->raw_floats * sizeof(float);
    SISIC_HIP(hipMemset(tr->grad, 0, bytes));
    SISIC_HIP(hipMemset(tr->adam_m, 0, bytes));
    SISIC_HIP(hipMemset(tr->adam_v, 0, bytes));
    tr->step = 0;
    unet_release_tape(u);
    SISIC_TRY(prepare_backward_weights(u, nullptr));
    SISIC_HIP(hipDeviceSynchronize());
    return SISIC_OK;
}

int sisic_unet_train_end(sisic_unet* u) {
    if (!u || !u->train) return SISIC_OK;
    (void)hipDeviceSynchronize();
    unet_release_tape(u);
    u->train.reset();
    return SISIC_OK;
}

int sisic_unet_set_dropout(sisic_unet* u, float p, uint64_t seed, uint32_t first_call) {
    SISIC_REQUIRE(u, "set_dropout: null handle");
    SISIC_REQUIRE(p >= 0.0f && p < 1.0f, "set_dropout: p = %g must be finite and in [0, 1)", (double)p);     // (false for a NaN)
    u->drop_p = p; u->drop_seed = seed; u->drop_call = first_call;
    return SISIC_OK;
}

uint32_t sisic_unet_dropout_next_call(const sisic_unet* u) { return u ? u->drop_call : 0; }

int sisic_unet_set_loss_weights(sisic_unet* u, const float* weights_host, int B) {
    SISIC_REQUIRE(u, "set_loss_weights: null handle");
    if (!weights_host || B == 0) {
        u->loss_w.clear();
        return SISIC_OK;
    }
    SISIC_REQUIRE(B > 0, "set_loss_weights: B = %d", B);
    for (int b = 0; b < B; ++b)
        SISIC_REQUIRE(std::isfinite(weights_host[b]), "set_loss_weights: weight %d is %g", b, (double)weights_host[b]);
    u->loss_w.assign(weights_host, weights_host + B);
    return SISIC_OK;
}

int sisic_unet_zero_grad(sisic_unet* u, void* stream) {
    SISIC_TRY(require_train(u, "zero_grad"));
    SISIC_HIP(hipMemsetAsync(u->train->grad, 0, u->raw_floats * sizeof(float), static_cast<hipStream_t>(stream)));
    return SISIC_OK;
}

int sisic_unet_train_forward(sisic_unet* u, const float* sample, const int64_t* timesteps, float* out, int B, int H, int W,
                             void* stream) {
    return train_forward(u, "train_forward", false, sample, timesteps, nullptr, out, B, H, W, stream);
}

int sisic_unet_train_forward_cond(sisic_unet* u, const float* sample, const int64_t* timesteps, const int64_t* class_labels,
                                  float* out, int B, int H, int W, void* stream) {
    return train_forward(u, "train_forward_cond", true, sample, timesteps, class_labels, out, B, H, W, stream);
}

int sisic_unet_backward(sisic_unet* u, const float* dout, void* stream) {
    SISIC_TRY(require_train(u, "backward"));
    TrainState* tr = u->train.get();
    if (!tr->has_tape) {
        set_error("backward: no recorded forward pass (call sisic_unet_train_forward first)");
        return SISIC_ESTATE;
    }
    SISIC_REQUIRE(dout, "backward: null output gradient");
    SISIC_HIP(hipSetDevice(u->ctx->device));
    Bwd b{u, tr, static_cast<hipStream_t>(stream), tr->B};
    const int rc = b.run(dout);
    unet_release_tape(u);  // blocks go back to the pool; the stream still orders later reuse behind the kernels above
    return rc;
}

int sisic_mse_loss(sisic_unet* u, const float* pred, const float* target, int64_t n, float grad_scale, float* loss_dev,
                   float* dpred, void* stream) {
    SISIC_TRY(require_train(u, "mse_loss"));
    const bool weighted = !u->loss_w.empty();
    const size_t B = weighted ? u->loss_w.size() : 1;
    SISIC_REQUIRE(!weighted || (pred && target && n > 0 && (size_t)n % B == 0),
                  "mse_loss: %lld elements are not %d equal samples (sisic_unet_set_loss_weights)", (long long)n, (int)B);
    return mse_objective(u, pred, target, nullptr, nullptr, (int)B, (size_t)n, grad_scale, loss_dev ? loss_dev : u->train->loss_dev, dpred,
                         static_cast<hipStream_t>(stream));
}

int sisic_add_noise(sisic_ctx* ctx, const float* x0, const float* noise, const float* sqrt_alpha_prod,
                    const float* sqrt_one_minus_alpha_prod, float* out, int B, int64_t per_sample, void* stream) {
    SISIC_REQUIRE(ctx && x0 && noise && sqrt_alpha_prod && sqrt_one_minus_alpha_prod && out && B > 0 && per_sample > 0,
                  "add_noise: bad arguments");
    return launch_add_noise(ctx, x0, noise, sqrt_alpha_prod, sqrt_one_minus_alpha_prod, out, B, (size_t)per_sample,
                            static_cast<hipStream_t>(stream));
}

// scaler.step(optimizer): one update launch; with found_inf the statistics pass, its 12-byte read-back and the skip decision first
int sisic_unet_optimizer_step(sisic_unet* u, double lr, double beta1, double beta2, double eps, float inv_scale, int* found_inf,
                              void* stream) {
    return optimizer_step(u, "optimizer_step", false, lr, beta1, beta2, eps, inv_scale, nullptr, found_inf, nullptr,
                          static_cast<hipStream_t>(stream));
}

// The same step with clipping and / or the EMA: the statistics pass always runs (norm, clip coefficient, found_inf).
int sisic_unet_optimizer_step_ext(sisic_unet* u, double lr, double beta1, double beta2, double eps, float inv_scale,
                                  const sisic_optim_ext* ext, int* found_inf, float* grad_norm_out, void* stream) {
    return optimizer_step(u, "optimizer_step_ext", true, lr, beta1, beta2, eps, inv_scale, ext, found_inf, grad_norm_out,
                          static_cast<hipStream_t>(stream));
}

int sisic_unet_train_step(sisic_unet* u, const float* images, const float* noise, const int64_t* timesteps,
                          const float* sqrt_alpha_prod, const float* sqrt_one_minus_alpha_prod, int B, int H, int W, double lr,
                          double beta1, double beta2, double eps, float loss_scale, float* loss_out, int* found_inf,
                          void* stream) {
    return train_step(u, {"train_step", false, false, images, noise, timesteps, nullptr, sqrt_alpha_prod, sqrt_one_minus_alpha_prod, B, H,
                          W, lr, beta1, beta2, eps, loss_scale, nullptr, loss_out, found_inf, nullptr, stream});
}

int sisic_unet_train_step_ext(sisic_unet* u, const float* images, const float* noise, const int64_t* timesteps,
                              const float* sqrt_alpha_prod, const float* sqrt_one_minus_alpha_prod, int B, int H, int W, double lr,
                              double beta1, double beta2, double eps, float loss_scale, const sisic_optim_ext* ext, float* loss_out,
                              int* found_inf, float* grad_norm_out, void* stream) {
    return train_step(u, {"train_step_ext", false, true, images, noise, timesteps, nullptr, sqrt_alpha_prod, sqrt_one_minus_alpha_prod, B,
                          H, W, lr, beta1, beta2, eps, loss_scale, ext, loss_out, found_inf, grad_norm_out, stream});
}

// ext == NULL: the plain step (no statistics pass unless found_inf asks; grad_norm_out is not written)
int sisic_unet_train_step_cond(sisic_unet* u, const float* images, const float* noise, const int64_t* timesteps,
                               const int64_t* class_labels, const float* sqrt_alpha_prod, const float* sqrt_one_minus_alpha_prod,
                               int B, int H, int W, double lr, double beta1, double beta2, double eps, float loss_scale,
                               const sisic_optim_ext* ext, float* loss_out, int* found_inf, float* grad_norm_out, void* stream) {
    return train_step(u, {"train_step_cond", true, ext != nullptr, images, noise, timesteps, class_labels, sqrt_alpha_prod,
                          sqrt_one_minus_alpha_prod, B, H, W, lr, beta1, beta2, eps, loss_scale, ext, loss_out, found_inf, grad_norm_out,
                          stream});
}

// ---- the EMA arena (diffusers' EMAModel: shadow parameters beside the trained ones)
int sisic_unet_ema_begin(sisic_unet* u) {
    SISIC_TRY(require_train(u, "ema_begin"));
    SISIC_TRY(require_not_swapped(u, "ema_begin"));
    TrainState* tr = u->train.get();
    SISIC_HIP(hipSetDevice(u->ctx->device));
    const size_t bytes = u->raw_floats * sizeof(float);
    if (!tr->ema) {
        void* q = nullptr;
        SISIC_HIP(hipMalloc(&q, bytes));
        SISIC_TRY(poison_fresh(q, bytes));
        tr->ema = static_cast<float*>(q);
    }
    SISIC_HIP(hipDeviceSynchronize());
    SISIC_HIP(hipMemcpy(tr->ema, u->raw, bytes, hipMemcpyDeviceToDevice));      // EMAModel.__init__: a copy of the parameters
    SISIC_HIP(hipDeviceSynchronize());
    return SISIC_OK;
}

int sisic_unet_ema_active(const sisic_unet* u) {
    if (!u || !u->train || !u->train->ema) return 0;
    return u->train->ema_swapped ? 2 : 1;
}

int sisic_unet_ema_step(sisic_unet* u, double ema_decay, void* stream) {
    SISIC_TRY(require_train(u, "ema_step"));
    SISIC_TRY(require_not_swapped(u, "ema_step"));
    TrainState* tr = u->train.get();
    if (!tr->ema) {
        set_error("ema_step: no EMA arena (call sisic_unet_ema_begin first)");
        return SISIC_ESTATE;
    }
    SISIC_HIP(hipSetDevice(u->ctx->device));
    return launch_ema(u->ctx, tr->ema, u->raw, u->raw_floats, ema_decay, static_cast<hipStream_t>(stream));
}

int sisic_unet_ema_swap(sisic_unet* u, void* stream) {
    SISIC_TRY(require_train(u, "ema_swap"));
    TrainState* tr = u->train.get();
    if (!tr->ema) {
        set_error("ema_swap: no EMA arena (call sisic_unet_ema_begin first)");
        return SISIC_ESTATE;
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    SISIC_HIP(hipSetDevice(u->ctx->device));
    // the raw arena keeps its address, so the batched repack plan stays valid: exchange the contents, re-derive the packed forms
    SISIC_TRY(launch_swap_arenas(u->ctx, u->raw, tr->ema, u->raw_floats, s));
    tr->ema_swapped = !tr->ema_swapped;
    return repack_after_update(u, s);
}

// sisic_unet_read / _write: tensor `index` of arena `what` to the host, or (write) from it; synchronises
static int unet_transfer(sisic_unet* u, const char* who, bool write, int what, int index, float* host, int64_t numel) {
    SISIC_REQUIRE(u, "%s: bad arguments", who);
    SISIC_TRY(u->dir.check_access(who, index, numel, host));
    SISIC_REQUIRE(!write || what != 0, "%s: parameters are set by sisic_unet_load (their packed forms must follow); what = 1 gradient, "
                                       "2 Adam m, 3 Adam v", who);
    float* base = u->raw;
    if (what != 0) {
        SISIC_TRY(require_train(u, who));
        TrainState* tr = u->train.get();                 // (4: the EMA arena, once sisic_unet_ema_begin has made it)
        base = what == 1 ? tr->grad : what == 2 ? tr->adam_m : what == 3 ? tr->adam_v : what == 4 ? tr->ema : nullptr;
    }
    SISIC_REQUIRE(base, "%s: what = %d (%s1 gradient, 2 Adam m, 3 Adam v)", who, what, write ? "" : "0 parameter, ");
    SISIC_HIP(hipSetDevice(u->ctx->device));
    SISIC_HIP(hipDeviceSynchronize());
    float* dev = base + u->offsets[index];
    SISIC_HIP(hipMemcpy(write ? dev : host, write ? host : dev, (size_t)numel * sizeof(float), write ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost));
    return SISIC_OK;
}

int sisic_unet_read(sisic_unet* u, int what, int index, float* out, int64_t numel) { return unet_transfer(u, "unet_read", false, what, index, out, numel); }

int sisic_unet_write(sisic_unet* u, int what, int index, const float* in, int64_t numel) {
    return unet_transfer(u, "unet_write", true, what, index, const_cast<float*>(in), numel);
}

int64_t sisic_unet_train_steps(const sisic_unet* u) { return (u && u->train) ? u->train->step : 0; }

// ---- single operators of the backward pass (parity-test surface): scratch is allocated per call
int sisic_conv2d_wgrad(sisic_ctx* ctx, const sisic_conv_args* f, const float* dy, float* dw, void* stream) {
    SISIC_REQUIRE(ctx && f && dy && dw, "conv2d_wgrad: null argument");
    SISIC_REQUIRE(f->upsample == 0 || f->upsample == 1, "conv2d_wgrad: upsample mode %d", f->upsample);
    hipStream_t s = static_cast<hipStream_t>(stream);
    WgradArgs a;
    a.in0 = f->in0; a.in1 = f->in1; a.c0 = f->c0; a.c1 = f->c1; a.B = f->B; a.Hin = f->Hin; a.Win = f->Win;
    a.ups = f->upsample; a.ksize = f->ksize; a.stride = f->stride;
    a.gn_scale = f->gn_scale; a.gn_shift = f->gn_shift; a.gn_silu = f->gn_silu;
    a.dy = dy; a.Cout = f->Cout; a.dw = dw;
    const size_t need = conv_wgrad_scratch_floats(a);
    void* part = nullptr;
    SISIC_HIP(hipMalloc(&part, need * sizeof(float)));
    SISIC_TRY(poison_fresh(part, need * sizeof(float)));
    const int rc = launch_conv_wgrad(ctx, a, static_cast<float*>(part), need, s);
    (void)hipStreamSynchronize(s);
    (void)hipFree(part);
    return rc;
}

int sisic_grad_stats(sisic_ctx* ctx, const float* g, int64_t n, float inv_scale, float max_norm, void* stats_dev, void* stream) {
    SISIC_REQUIRE(ctx && g && stats_dev && n > 0, "grad_stats: bad arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    void* scratch = nullptr;
    SISIC_HIP(hipMalloc(&scratch, grad_stats_scratch_bytes()));
    SISIC_TRY(poison_fresh(scratch, grad_stats_scratch_bytes()));
    const int rc = launch_grad_stats(ctx, g, (size_t)n, inv_scale, max_norm, static_cast<GradStats*>(stats_dev), scratch, s);
    (void)hipStreamSynchronize(s);
    (void)hipFree(scratch);
    return rc;
}

int sisic_adam_ema(sisic_ctx* ctx, float* p, const float* g, float* m, float* v, float* ema, int64_t n, double lr, double beta1,
                   double beta2, double eps, int64_t step, float inv_scale, const void* stats_dev, double ema_decay, void* stream) {
    SISIC_REQUIRE(ctx && p && g && m && v && n > 0 && step >= 1, "adam_ema: bad arguments");
    hipStream_t s = static_cast<hipStream_t>(stream);
    return launch_adam_ema(ctx, p, g, m, v, ema, (size_t)n, lr, beta1, beta2, eps, step, inv_scale,
                           static_cast<const GradStats*>(stats_dev), ema_decay, s);
}

int sisic_attention_bwd(sisic_ctx* ctx, const float* qkv, const float* o, const float* dO, float* dqkv, int B, int C, int N,
                        int head_dim, void* stream) {
    SISIC_REQUIRE(ctx, "attention_bwd: null context");
    return launch_attention_bwd(ctx, qkv, o, dO, dqkv, B, C, N, head_dim, static_cast<hipStream_t>(stream));
}

int sisic_groupnorm_bwd(sisic_ctx* ctx, const float* da, const float* x, int B, int C, int HW, int groups, float eps,
                        const float* gamma, const float* beta, int silu, float* dx_accum, float* dgamma, float* dbeta,
                        void* stream) {
    SISIC_REQUIRE(ctx && da && x && gamma && beta && dx_accum && dgamma && dbeta, "groupnorm_bwd: null argument");
    SISIC_REQUIRE(B > 0 && C > 0 && HW > 0 && groups > 0 && C % groups == 0, "groupnorm_bwd: bad shape");
    hipStream_t s = static_cast<hipStream_t>(stream);
    void* p = nullptr;
    const size_t n = (size_t)4 * B * C + (size_t)2 * B * groups;
    SISIC_HIP(hipMalloc(&p, n * sizeof(float)));
    SISIC_TRY(poison_fresh(p, n * sizeof(float)));
    float* scale = static_cast<float*>(p);
    float* shift = scale + (size_t)B * C;
    float* sums = shift + (size_t)B * C;
    float* mr = sums + (size_t)2 * B * C;
    int rc = launch_gn_stats(ctx, x, C, nullptr, 0, B, HW, groups, eps, gamma, beta, scale, shift, s, mr);
    if (rc == SISIC_OK)
        rc = launch_gn_bwd(ctx, da, x, C, nullptr, 0, B, HW, groups, scale, shift, mr, gamma, silu, sums, dx_accum, nullptr, dgamma,
                           dbeta, s);
    (void)hipStreamSynchronize(s);
    (void)hipFree(p);
    return rc;
}

}  // extern "C"
