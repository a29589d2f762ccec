// UNet engine: the MI355X-native replacement of the reference's
//     self.unet(z_in, t_in, encoder_hidden_states=c_embed[, added_cond_kwargs])['sample']
// (latent_diffusion.py:146-156, latent_sdxl.py:170-183).
//
// Architecture follows diffusers-0.27.1 UNet2DConditionModel semantics for the
// SD1.5 / SDXL configs: conv_in, time (+ text_time) embedding,
// {ResnetBlock2D, Transformer2DModel} down / mid / up blocks with skip concat,
// GroupNorm-SiLU-conv_out.  Weights are loaded by their diffusers state-dict keys
// and repacked once into the layouts the kernels want; the forward is a static
// launch plan (vector of closures) over preallocated, shape-keyed activation
// buffers in halo-padded NHWC fp16 - no allocation, no host sync, one stream.
#include "engine_base.h"
#include "../../include/cfgpp_ip_plus.h"
#include "../../include/cfgpp_lcm.h"
#include "../../include/cfgpp_regions.h"
#include "../../include/cfgpp_regions_soft.h"
#include "freeu.h"

struct cfgpp_unet : EngineBase {
    cfgpp_unet_config cfg;
    int device = 0;
    bool finalized = false;

    std::vector<Op> ctx_plan;       // set_context (cross-attention K/V, added-condition embedding)
    // forward-time inputs (pointers patched per call)
    const void* in_z = nullptr; int in_z_half = 0; int in_z_rows = 0; float in_t = 0.f; void* out_eps = nullptr;
    const float* in_t_dev = nullptr;        // non-null: the timestep sinusoid reads *in_t_dev (graph replay) instead of in_t
    // inpaint UNets (in_channels > out_channels): the step-invariant extra input channels (mask + masked-image latent), fp16
    // [cond_rows][in - out][H][W] in an engine-owned buffer whose address never changes (captured graphs stay valid)
    half_t* d_cond = nullptr; int cond_rows = 0;
    // whole-step graph replay (cfgpp_sample_graph_ddim): per-step scalar table, current-step block, step counter, the one cached graph
    float* d_step_tab = nullptr; int step_tab_cap = 0; float* d_step_cur = nullptr; int* d_step_idx = nullptr;
    hipStream_t cap_stream = nullptr;
    struct GraphKey { const void* z; void* z0t; void* eps; const void* euc; const void* ec; int z_half, z_rows, rows, tw, rn; float lam; long n; int tuned_serial; int cond_rows;
                      int ip_active = 0, ip_n_img = 0; unsigned ip_scale_bits = 0;         // the adapter state the captured launches baked in
                      int ctx_tokens = 77;          // the text context's token count: the captured cross-attention launches bake in nk, the kernel and its LDS size
                      int freeu_on = 0; unsigned freeu_bits[4] = {0, 0, 0, 0}; };     // FreeU state: the captured edits bake in s / b (off: no such launches)
    struct Graph { GraphKey key; hipGraph_t graph; hipGraphExec_t exec; };
    std::vector<Graph> graphs;              // most recently used last; at most 4 (an invert + edit job alternates between two)
    int tuned_serial = 0;                   // bumps whenever the pins of the current batch change (a graph bakes the tiles it captured)
    // ---- shared CFG prefix.  A CFG call runs rows = 2 * z_rows with row r reading latent r % z_rows; without add_embedding the
    // time embedding is one vector for every row, so rows r and r + z_rows first differ at the first cross-attention (the text
    // context).  The plan ops from down_blocks.0.resnets.0 to the attn2.to_q projection of down_blocks.0.attentions.0 (plan_share
    // == 1) then run on the leading z_rows rows only and one fan-out launch (plan_share == 2) copies the three live tensors - the
    // token stream, the head-major Q and the resnet output the transformer's proj_out adds - onto the upper rows.
    int prefix_ops = 0;                     // plan ops marked 1 (0: this net has no shareable prefix - SDXL)
    double prefix_macs_per_row = 0;         // their MACs per batch row (matmuls and attention)
    int ran_shared = -1;                    // mode of the most recent forward / profile (-1: none yet)
    bool shares(int rows, int z_rows) const;
    // run-time mode of a call: bumps tuned_serial when it differs from the last one, so no captured graph replays the other plan
    bool enter_call(int rows, int z_rows) {
        const bool sh = shares(rows, z_rows);
        if (ran_shared != (int)sh) { if (ran_shared >= 0) ++tuned_serial; ran_shared = (int)sh; }
        return sh;
    }
    static void destroy(Graph& g) { if (g.exec) hipGraphExecDestroy(g.exec); if (g.graph) hipGraphDestroy(g.graph); g.exec = nullptr; g.graph = nullptr; }
    void drop_graphs() { for (auto& g : graphs) destroy(g); graphs.clear(); }
    ~cfgpp_unet() { drop_graphs(); if (cap_stream) hipStreamDestroy(cap_stream); for (auto& a : ip_allocs) hipFree(a.first); }
    // context inputs
    const half_t* ctx_ehs = nullptr; int ctx_rows = 0; int ctx_tokens = 77;
    // longest text context the cross-attention buffers are built for (cfgpp_unet_set_max_tokens, before finalize): 77 * j, j <= 4.
    // ck / cvt of every block have ck_pad = max(128, round_up(max_tokens, 64)) key slots; a context of fewer tokens leaves slots
    // [tokens, ck_pad) as an earlier, longer context wrote them - finite values that every attention kernel on the path masks
    // (P = 0) or never loads, so nothing is cleared.
    int max_tokens = 77;
    const half_t* ctx_text = nullptr; const float* ctx_tids = nullptr; int ctx_cond_rows = 0;
    bool ctx_set = false;
    // ---- regional prompts (include/cfgpp_regions.h: cfgpp_unet_set_regions).  regions = 0: off, the plain engine.  regions = R =
    // 2 .. 4: the context holds R chunks of 77 tokens and every cross-attention op calls cfgpp_op_attention_region with the region
    // map of its level - uint8 [region_map_rows][q_pad of the level], pads 0, in buffers finalize allocates when max_tokens > 77
    // (d_region_ids[level], max_rows x q_pad bytes each) and set_regions fills from the host, once per job.
    int regions = 0, region_map_rows = 0;
    unsigned char* d_region_ids[4] = {nullptr, nullptr, nullptr, nullptr};
    int region_h[4] = {0, 0, 0, 0}, region_w[4] = {0, 0, 0, 0};
    // ---- soft regional prompts (include/cfgpp_regions_soft.h).  soft_enabled (cfgpp_unet_enable_region_weights, before finalize) makes
    // finalize allocate, next to the id maps, one fp32 weight buffer per level, [max_rows][4][q_pad of the level].  soft_regions = R
    // = 2 .. 4 (cfgpp_unet_set_region_weights): every cross-attention op calls cfgpp_op_attention_region_soft with its level's weights,
    // [soft_map_rows][R][q_pad], pads 0.  Soft weights and the hard id map are exclusive: setting one clears the other.
    bool soft_enabled = false;
    int soft_regions = 0, soft_map_rows = 0;
    float* d_region_w[4] = {nullptr, nullptr, nullptr, nullptr};

    // time-embedding scratch
    float* d_sin_t = nullptr; float* d_emb_h = nullptr; float* d_emb_t = nullptr; float* d_emb = nullptr;
    float* d_temb_all = nullptr; int temb_total = 0;
    float* d_add_in = nullptr; float* d_add_h = nullptr; float* d_aug = nullptr;
    // guidance-embedded UNets (include/cfgpp_lcm.h: cfgpp_unet_set_time_cond, before finalize): time_cond = time_cond_proj_dim.
    // cfgpp_unet_guidance_embedding computes, once per job, d_time_add = linear_1.weight x (cond_proj x w_emb) into an engine-owned
    // buffer whose address never changes; the forward's linear_1 launch takes it as its addend (it lands before the SiLU), so
    // linear_1(sinusoid(t) + cond_proj(w_emb)) costs the forward no launch of its own.
    int time_cond = 0; bool time_cond_set = false;
    half_t* w_cond = nullptr; half_t* w_time1 = nullptr;
    float* d_w_emb = nullptr; float* d_cond_vec = nullptr; float* d_time_add = nullptr;
    std::vector<float> h_w_emb;             // the host copy the upload reads (stable address)

    // transformer scratch (token-major)
    half_t *tok_x = nullptr, *tok_ln = nullptr, *tok_attn = nullptr, *tok_ff = nullptr;
    // head-major Q / K / V^T scratch, ONE SET PER LEVEL: a level has fixed (heads, tokens, d), so the
    // zero padding of the head dim (d..dp) is never overwritten by a differently shaped user.
    half_t *hq[4] = {nullptr, nullptr, nullptr, nullptr}, *hk[4] = {nullptr, nullptr, nullptr, nullptr},
           *hvt[4] = {nullptr, nullptr, nullptr, nullptr};

    // ---- ControlNet.  control = this engine IS a ControlNet (cfgpp_unet_create with out_channels = 0): conv_in adds the embedded control image,
    // the plan ends with the zero convolutions into the persistent residuals ctrl_res (the skips' order, then the mid block's)
    bool control = false;
    std::vector<int> embed_ch;              // ControlNetConditioningEmbedding block_out_channels
    std::vector<Op> img_plan;               // the embedding (cfgpp_unet_image_condition), rows = image rows
    const void* img_in = nullptr; int img_in_half = 0;
    half_t* d_img_emb = nullptr; int img_rows = 0;      // embedded image: halo-padded NHWC [max_rows][H+2][W+2][c0], fixed address
    std::vector<Tensor> ctrl_res;
    // controlled UNet: the tensors the residuals are added to (skips, then the mid-block output), the attached net and its scale
    std::vector<Tensor> ctrl_dst;
    cfgpp_unet* ctrl = nullptr; float ctrl_scale = 0.f;
    CnAddEntry* d_ctrl_tab = nullptr; long ctrl_max_n8 = 0;

    // ---- FreeU (cfgpp_unet_set_freeu; EngineBase::freeu_on): {s, b} of up_blocks.0 / up_blocks.1 and the twiddle table of each
    // block's plane size (freeu_twiddles, built by finalize: the setter allocates nothing)
    float freeu_s[2] = {1.f, 1.f}, freeu_b[2] = {1.f, 1.f};
    float* d_freeu_tw[2] = {nullptr, nullptr};

    // ---- IP-Adapter (cfgpp_unet_ip_load / cfgpp_unet_image_context).  Every cross-attention block keeps its text K / V^T in
    // key slots [0, 77) of ck / cvt (ck_pad = 128 slots); the image tokens' K / V^T go into slots [96, 96 + n_img) of the same
    // buffers and the block's attention op becomes the decoupled form while the adapter is active.
    static constexpr int IP_SLOT = 96, IP_MAX = 32;
    struct IpBlock {
        std::string name;               // "<diffusers block>.attn2"
        int C, nheads, d, dp, tok; half_t* ck; half_t* cvt;
        size_t plan_idx;                // the block's cross-attention op in `plan`
        half_t* wkv = nullptr;          // [to_k_ip ; to_v_ip] = [2C][cross_dim] fp16 (adapter memory)
        bool has_k = false, has_v = false;
    };
    std::vector<IpBlock> ip_blocks;     // plan order
    int ip_ck_pad = 0;
    half_t* ip_wproj = nullptr; float* ip_bproj = nullptr; float* ip_ng = nullptr; float* ip_nb = nullptr;
    long ip_proj_rows = 0, ip_bias_rows = 0; int ip_embed = 0;      // image_proj.proj: [n_img * cross_dim][embed_dim]
    half_t* ip_proj_out = nullptr; half_t* ip_tok = nullptr; long ip_tok_cap = 0;   // proj output / LayerNorm output, [rows][n_img][cross_dim]
    std::vector<std::pair<void*, size_t>> ip_allocs;
    bool ip_active = false; int ip_n_img = 0; float ip_scale = 0.f;
    const void* ip_src = nullptr; int ip_rows = 0;                  // the embeds the slots were computed from (by address) and their rows
    void* ip_malloc(size_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
        ip_allocs.push_back(std::make_pair(p, bytes)); dev_bytes += (double)bytes;
        return p;
    }
    void ip_free(void* p) {
        for (size_t i = 0; i < ip_allocs.size(); ++i)
            if (ip_allocs[i].first == p) { hipFree(p); dev_bytes -= (double)ip_allocs[i].second; ip_allocs.erase(ip_allocs.begin() + i); return; }
    }
    // the image keys count in the FLOPs and in the profiler's tags only while the adapter is active
    double ip_macs_per_key = 0;         // sum over blocks of 2 * heads * tokens * d
    void ip_set_active(bool on, int n_img, float scale) {
        ip_active = on; ip_n_img = on ? n_img : 0; ip_scale = on ? scale : 0.f;
        for (const IpBlock& b : ip_blocks) {
            const double per_key = 2.0 * (double)b.nheads * b.tok * b.d;
            const std::string desc = "cross_attn heads=" + std::to_string(b.nheads) + " N=" + std::to_string(b.tok) + " d=" + std::to_string(b.d);
            plan_macs[b.plan_idx] = regions ? per_key * 77 : per_key * (ctx_tokens + ip_n_img);      // a regional row attends to its own 77 keys
            plan_desc[b.plan_idx] = on ? desc + " ip=" + std::to_string(n_img) : ctx_tokens != 77 ? desc + " keys=" + std::to_string(ctx_tokens) : desc;
            if (regions) plan_desc[b.plan_idx] += " regions=" + std::to_string(regions);
            // soft regions: a row may weigh every region, so all 77 R keys are counted (what a fully mixed map runs)
            if (soft_regions) plan_desc[b.plan_idx] += " soft_regions=" + std::to_string(soft_regions);
        }
    }
    // the profiler's tags of the cross-attention ops follow the token count of the current context
    void retag_cross() { if (plan_macs.size() == plan.size()) ip_set_active(ip_active, ip_n_img, ip_scale); }
    // ---- the Resampler image projection of the "plus" adapters (include/cfgpp_ip_plus.h), an optional part of the adapter state.
    // ip_kind: which image projection this adapter has - fixed by the first image_proj.* tensor after a drop.
    enum { IP_NONE = 0, IP_LINEAR = 1, IP_RESAMPLER = 2 };
    int ip_kind = IP_NONE;
    enum { RG_LATENTS, RG_PIN_W, RG_PIN_B, RG_POUT_W, RG_POUT_B, RG_NOUT_W, RG_NOUT_B, RG_COUNT };
    enum { RL_N1_W, RL_N1_B, RL_N2_W, RL_N2_B, RL_Q, RL_KV, RL_OUT, RL_FN_W, RL_FN_B, RL_FF1, RL_FF2, RL_COUNT };
    static constexpr int RES_MAX_DEPTH = 8;
    struct Resampler {
        void* g[RG_COUNT] = {};                         // fp16 matrices [N][K]; fp32 biases, norms and latents
        void* l[RES_MAX_DEPTH][RL_COUNT] = {};
        int E = 0, D = 0, nq = 0, inner = 0, ff = 0;    // geometry as the tensors loaded so far fixed it (0: not yet)
        // activations, fp16 (ip_malloc: adapter memory).  xs = {x, xn, kv_x}, sized by (max_rows, S_cap); the rest by max_rows
        half_t* xs = nullptr; int S_cap = 0;
        half_t* ls = nullptr;
    } res;
    int ip_seq = 0;                                     // Resampler: the seq of the hidden states the slots were computed from
    void ip_drop() {
        if (plan_macs.size() == plan.size()) ip_set_active(false, 0, 0.f);
        while (!ip_allocs.empty()) ip_free(ip_allocs.back().first);
        for (IpBlock& b : ip_blocks) { b.wkv = nullptr; b.has_k = b.has_v = false; }
        ip_wproj = nullptr; ip_bproj = nullptr; ip_ng = nullptr; ip_nb = nullptr; ip_proj_out = nullptr; ip_tok = nullptr;
        ip_proj_rows = ip_bias_rows = 0; ip_embed = 0; ip_tok_cap = 0; ip_src = nullptr; ip_rows = 0;
        res = Resampler(); ip_kind = IP_NONE; ip_seq = 0;
    }
};

static int g_share_prefix = 1;
bool cfgpp_unet::shares(int rows, int z_rows) const { return g_share_prefix && prefix_ops > 0 && rows == 2 * z_rows; }

namespace {

void build_param_table(cfgpp_unet* u) {
    const cfgpp_unet_config& c = u->cfg;
    const int L = c.num_levels;
    const long c0 = c.block_out_channels[0], temb = 4 * c0;
    expect_conv(u, "conv_in", c0, c.in_channels, 3);
    expect_linear(u, "time_embedding.linear_1", temb, c0);
    expect_linear(u, "time_embedding.linear_2", temb, temb);
    if (c.addition_embed) {
        const long in = (long)c.addition_time_embed_dim * 6 + c.addition_pooled_dim;
        expect_linear(u, "add_embedding.linear_1", temb, in);
        expect_linear(u, "add_embedding.linear_2", temb, temb);
    }
    long ch = c0;
    for (int i = 0; i < L; ++i) {
        const long co = c.block_out_channels[i];
        const std::string p = "down_blocks." + std::to_string(i);
        for (int j = 0; j < c.layers_per_block; ++j) {
            expect_resnet(u, p + ".resnets." + std::to_string(j), ch, co, temb);
            if (c.level_has_attn[i])
                expect_transformer(u, p + ".attentions." + std::to_string(j), co, c.transformer_depth[i], c.cross_attention_dim);
            ch = co;
        }
        if (i != L - 1) expect_conv(u, p + ".downsamplers.0.conv", co, co, 3);
    }
    const long cm = c.block_out_channels[L - 1];
    expect_resnet(u, "mid_block.resnets.0", cm, cm, temb);
    expect_transformer(u, "mid_block.attentions.0", cm, c.transformer_depth[L - 1], c.cross_attention_dim);
    expect_resnet(u, "mid_block.resnets.1", cm, cm, temb);
    if (u->control) {
        // ControlNetConditioningEmbedding: conv_in, then per level a stride-1 and a stride-2 conv, conv_out to c0
        const std::vector<int>& e = u->embed_ch;
        const std::string q = "controlnet_cond_embedding.";
        expect_conv(u, q + "conv_in", e[0], 3, 3);
        for (size_t i = 0; i + 1 < e.size(); ++i) {
            expect_conv(u, q + "blocks." + std::to_string(2 * i), e[i], e[i], 3);
            expect_conv(u, q + "blocks." + std::to_string(2 * i + 1), e[i + 1], e[i], 3);
        }
        expect_conv(u, q + "conv_out", c0, e.back(), 3);
        // zero convolutions: one per skip connection (conv_in, every down resnet / attention, every downsampler), then the mid block
        int k = 0;
        expect_conv(u, "controlnet_down_blocks." + std::to_string(k++), c0, c0, 1);
        for (int i = 0; i < L; ++i) {
            const long co = c.block_out_channels[i];
            for (int j = 0; j < c.layers_per_block; ++j) expect_conv(u, "controlnet_down_blocks." + std::to_string(k++), co, co, 1);
            if (i != L - 1) expect_conv(u, "controlnet_down_blocks." + std::to_string(k++), co, co, 1);
        }
        expect_conv(u, "controlnet_mid_block", cm, cm, 1);
        return;                              // no up path, no conv_out
    }
    // up blocks (diffusers: reversed channels; layers_per_block+1 resnets each)
    long prev = cm;
    for (int i = 0; i < L; ++i) {
        const int lvl = L - 1 - i;
        const long co = c.block_out_channels[lvl];
        const long cin_lvl = c.block_out_channels[std::max(lvl - 1, 0)];
        const std::string p = "up_blocks." + std::to_string(i);
        for (int j = 0; j < c.layers_per_block + 1; ++j) {
            const long skip = (j == c.layers_per_block) ? cin_lvl : co;
            const long rin = (j == 0 ? prev : co) + skip;
            expect_resnet(u, p + ".resnets." + std::to_string(j), rin, co, temb);
            if (c.level_has_attn[lvl])
                expect_transformer(u, p + ".attentions." + std::to_string(j), co, c.transformer_depth[lvl], c.cross_attention_dim);
        }
        if (i != L - 1) expect_conv(u, p + ".upsamplers.0.conv", co, co, 3);
        prev = co;
    }
    expect_norm(u, "conv_norm_out", c0);
    expect_conv(u, "conv_out", c.out_channels, c0, 3);
}

// ---------------------------------------------------------------------------
// weight repacking (host) + upload
// ---------------------------------------------------------------------------
struct ResW {
    float *n1g, *n1b, *n2g, *n2b, *b1, *b2, *bsc;
    half_t *w1, *w2, *wsc;
    int temb_off;   // column offset in temb_all
    int cin, cout;
};

// ControlNet tail of the plan (control mode): the 1x1 zero convolutions of every skip and of the mid-block output into persistent
// residual tensors (the controlled UNet's skip layout, so the add is elementwise), and the embedding plan of the control image
// (ControlNetConditioningEmbedding: SiLU after every conv but conv_out), whose output is conv_in's addend.
int controlnet_tail(cfgpp_unet* u, Builder& B, Plan& P, const std::vector<Tensor>& skips, const Tensor& mid) {
    const cfgpp_unet_config& c = u->cfg;
    const int R = c.max_rows, c0 = c.block_out_channels[0];
    auto persist = [&](int H, int W, int C) {
        Tensor t; t.H = H; t.W = W; t.C = C;
        t.p = (half_t*)u->dmalloc((size_t)R * (H + 2) * (W + 2) * C * sizeof(half_t));      // zeroed: the halo stays zero
        return t;
    };
    for (size_t k = 0; k <= skips.size(); ++k) {
        const Tensor& src = k < skips.size() ? skips[k] : mid;
        const std::string key = k < skips.size() ? "controlnet_down_blocks." + std::to_string(k) : std::string("controlnet_mid_block");
        half_t* w = B.linear(key + ".weight"); float* b = B.f32(key + ".bias");
        Tensor r = persist(src.H, src.W, src.C);
        CFGPP_REQUIRE(r.p, "finalize: hipMalloc failed");
        P.conv1x1(src, nullptr, r, w, b);
        u->ctrl_res.push_back(r);
    }
    // ---- embedding: direct convolutions at the image size, then conv_out on the implicit GEMM ----
    const std::vector<int>& e = u->embed_ch;
    const int n = (int)e.size();
    const std::string q = "controlnet_cond_embedding.";
    struct Layer { std::string key; int ci, co, stride; };
    std::vector<Layer> layers;
    layers.push_back({q + "conv_in", 3, e[0], 1});
    for (int i = 0; i + 1 < n; ++i) {
        layers.push_back({q + "blocks." + std::to_string(2 * i), e[i], e[i], 1});
        layers.push_back({q + "blocks." + std::to_string(2 * i + 1), e[i], e[i + 1], 2});
    }
    // dense NHWC ping-pong scratch for every layer but the last direct one, which writes conv_out's halo-padded input
    long scratch = 1;
    {
        int h = c.sample_h << (n - 1), w = c.sample_w << (n - 1);
        for (size_t l = 0; l + 1 < layers.size(); ++l) {
            if (layers[l].stride == 2) { h = (h - 1) / 2 + 1; w = (w - 1) / 2 + 1; }
            scratch = std::max(scratch, (long)R * h * w * layers[l].co);
        }
    }
    half_t* buf[2] = {(half_t*)u->dmalloc((size_t)scratch * sizeof(half_t), false), (half_t*)u->dmalloc((size_t)scratch * sizeof(half_t), false)};
    Tensor pre = persist(c.sample_h, c.sample_w, e.back());
    CFGPP_REQUIRE(buf[0] && buf[1] && pre.p, "finalize: hipMalloc failed");
    cfgpp_unet* uu = u;
    int h = c.sample_h << (n - 1), w = c.sample_w << (n - 1);
    for (size_t l = 0; l < layers.size(); ++l) {
        const Layer& ly = layers[l];
        HostParam* pw = B.get(ly.key + ".weight");
        CFGPP_REQUIRE(pw, "finalize: %s", B.err.c_str());
        std::vector<float> r((size_t)9 * ly.ci * ly.co);          // OIHW -> [tap][ci][co]
        for (int o = 0; o < ly.co; ++o) for (int i = 0; i < ly.ci; ++i) for (int t = 0; t < 9; ++t)
            r[((size_t)t * ly.ci + i) * ly.co + o] = (float)pw->h[((size_t)o * ly.ci + i) * 9 + t];
        B.drop(ly.key + ".weight");
        float* dw = B.upload(r); float* db = B.f32(ly.key + ".bias");
        const bool last = l + 1 == layers.size();
        const half_t* in = l == 0 ? nullptr : buf[(l - 1) & 1];
        half_t* out = last ? pre.p : buf[l & 1];
        const int hi = h, wi = w, ci = ly.ci, co = ly.co, st = ly.stride, first = l == 0;
        u->img_plan.push_back([=](hipStream_t s, int rows) {
            return cfgpp_op_cn_conv3x3(first ? uu->img_in : in, first ? (uu->img_in_half ? 1 : 2) : 0, out, last ? 1 : 0, dw, db, rows, ci,
                                       co, hi, wi, st, 1, s);
        });
        if (st == 2) { h = (h - 1) / 2 + 1; w = (w - 1) / 2 + 1; }
    }
    CFGPP_REQUIRE(h == c.sample_h && w == c.sample_w, "finalize: internal error, the embedding ends at %d x %d", h, w);
    {
        half_t* wo = B.conv3(q + "conv_out.weight"); float* bo = B.f32(q + "conv_out.bias");
        Tensor dst; dst.p = u->d_img_emb; dst.H = c.sample_h; dst.W = c.sample_w; dst.C = c0;
        Plan PI{u, &B, &u->img_plan};
        const double macs = u->macs_per_row;
        PI.conv3x3(pre, dst, wo, bo, 1, nullptr, 0, nullptr);
        u->macs_per_row = macs;               // once per job: not part of a forward's FLOPs
    }
    CFGPP_REQUIRE(B.ok, "finalize: %s", B.err.c_str());
    return 0;
}

}  // namespace

// ---------------------------------------------------------------------------
extern "C" {

static cfgpp_unet* unet_new(const cfgpp_unet_config* cfg, int device_id, const int* embed, int n_embed) {
    if (!cfg) { cfgpp_set_error("unet_create: null config"); return nullptr; }
    if (cfg->num_levels < 1 || cfg->num_levels > 4 || cfg->layers_per_block < 1 || cfg->max_rows < 1) {
        cfgpp_set_error("unet_create: bad config"); return nullptr;
    }
    for (int i = 0; i < cfg->num_levels; ++i) {
        const int c = cfg->block_out_channels[i];
        if (c % 64 != 0 || c % cfg->norm_groups != 0) { cfgpp_set_error("unet_create: channels %d must be a multiple of 64 and of norm_groups", c); return nullptr; }
        if (cfg->level_has_attn[i]) {
            const int d = c / cfg->num_heads[i];
            if (c % cfg->num_heads[i] != 0 || d % 4 != 0 || d > 160) { cfgpp_set_error("unet_create: head dim %d unsupported", d); return nullptr; }
        }
    }
    if (cfg->cross_attention_dim % 64 != 0) { cfgpp_set_error("unet_create: cross_attention_dim must be a multiple of 64"); return nullptr; }
    if (!embed && cfg->in_channels > cfg->out_channels && cfg->in_channels > 16) {
        cfgpp_set_error("unet_create: in_channels=%d out_channels=%d (an inpaint UNet takes at most 16 input channels)", cfg->in_channels,
                        cfg->out_channels);
        return nullptr;
    }
    if ((cfg->sample_h % (1 << (cfg->num_levels - 1))) || (cfg->sample_w % (1 << (cfg->num_levels - 1)))) {
        cfgpp_set_error("unet_create: sample size %d x %d must be divisible by 2^(levels-1) = %d", cfg->sample_h, cfg->sample_w,
                        1 << (cfg->num_levels - 1));
        return nullptr;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device_id) {
        cfgpp_set_error("unet_create: no HIP device %d (found %d) - the HIP path has no CPU fallback", device_id, ndev);
        return nullptr;
    }
    if (cfgpp_claim_device(device_id)) return nullptr;
    if (hipSetDevice(device_id) != hipSuccess) { cfgpp_set_error("unet_create: hipSetDevice failed"); return nullptr; }
    cfgpp_unet* u = new cfgpp_unet();
    u->cfg = *cfg; u->device = device_id; u->max_rows = cfg->max_rows; u->norm_groups = cfg->norm_groups;
    if (embed) { u->control = true; u->embed_ch.assign(embed, embed + n_embed); }
    build_param_table(u);
    return u;
}

cfgpp_unet* cfgpp_unet_create(const cfgpp_unet_config* cfg, int device_id) {
    if (cfg && cfg->out_channels == 0) {
        // a ControlNet: diffusers' ControlNetConditioningEmbedding with its default conditioning_embedding_out_channels
        static const int embed[4] = {16, 32, 96, 256};
        if (cfg->in_channels < 1 || cfg->in_channels > 8) {
            cfgpp_set_error("unet_create: ControlNet (out_channels = 0) with in_channels=%d (1 .. 8 latent channels)", cfg->in_channels);
            return nullptr;
        }
        return unet_new(cfg, device_id, embed, 4);
    }
    return unet_new(cfg, device_id, nullptr, 0);
}


void cfgpp_unet_destroy(cfgpp_unet* u) {
    if (!u) return;
    delete u;
}

int cfgpp_unet_load_tensor(cfgpp_unet* u, const char* key, const void* host, int dtype, const long* shape, int ndim) {
    CFGPP_REQUIRE(u && key && host && shape, "load_tensor: null argument");
    CFGPP_REQUIRE(!u->finalized, "load_tensor: context already finalized");
    auto it = u->params.find(key);
    if (it == u->params.end()) { cfgpp_set_error("load_tensor: unknown key %s", key); return -3; }
    HostParam& p = it->second;
    long n = 1; for (int i = 0; i < ndim; ++i) n *= shape[i];
    CFGPP_REQUIRE(n == p.numel(), "load_tensor: %s has %ld elements, expected %ld", key, n, p.numel());
    if (ndim == 4) { p.shape.assign(shape, shape + 4); }   // keep OIHW (conv1x1 vs linear both fine)
    if (p.is_matrix && !(std::string(key) == "conv_in.weight")) {
        p.h.resize(n);
        if (dtype == 0) { const float* s = (const float*)host; for (long i = 0; i < n; ++i) p.h[i] = (half_t)s[i]; }
        else std::memcpy(p.h.data(), host, n * sizeof(half_t));
    } else {
        p.f.resize(n);
        if (dtype == 0) std::memcpy(p.f.data(), host, n * sizeof(float));
        else { const half_t* s = (const half_t*)host; for (long i = 0; i < n; ++i) p.f[i] = (float)s[i]; }
    }
    p.loaded = true;
    return 0;
}

int cfgpp_unet_missing(cfgpp_unet* u) {
    if (!u) return -1;
    int n = 0; std::string names;
    for (auto& kv : u->params) if (!kv.second.loaded) { if (n < 8) names += kv.first + " "; ++n; }
    if (n) cfgpp_set_error("missing %d parameters: %s...", n, names.c_str());
    return n;
}

int cfgpp_unet_finalize(cfgpp_unet* u) {
    CFGPP_REQUIRE(u, "finalize: null");
    CFGPP_REQUIRE(!u->finalized, "finalize: already finalized");
    if (cfgpp_unet_missing(u) != 0) { const std::string m = cfgpp_last_error(); cfgpp_set_error("finalize: %s", m.c_str()); return -2; }
    CFGPP_HIP_CHECK(hipSetDevice(u->device));
    const cfgpp_unet_config& c = u->cfg;
    const int L = c.num_levels, R = c.max_rows;
    const int c0 = c.block_out_channels[0], temb_dim = 4 * c0;
    Builder B{u};
    Plan P{u, &B, &u->plan};
    Plan PC{u, &B, &u->ctx_plan};

    // ---- scratch sizing ----
    long max_tok_c = 0, max_ff = 0;
    {
        int H = c.sample_h, W = c.sample_w;
        for (int i = 0; i < L; ++i) {
            const long C = c.block_out_channels[i];
            if (c.level_has_attn[i] || i == L - 1) {
                const long tok = (long)H * W;
                const int d = (int)(C / c.num_heads[i]), dp = round_up(d, 32);
                max_tok_c = std::max(max_tok_c, tok * C);
                max_ff = std::max(max_ff, tok * 4 * C);
                u->hq[i] = (half_t*)u->dmalloc((size_t)R * c.num_heads[i] * round_up((int)tok, 128) * dp * 2);
                u->hk[i] = (half_t*)u->dmalloc((size_t)R * c.num_heads[i] * round_up((int)tok, 128) * dp * 2);
                u->hvt[i] = (half_t*)u->dmalloc((size_t)R * c.num_heads[i] * dp * round_up((int)tok, 64) * 2);
                CFGPP_REQUIRE(u->hq[i] && u->hk[i] && u->hvt[i], "finalize: hipMalloc failed");
                if (cfgpp_op_attention_prepare_vt(u->hvt[i], R * c.num_heads[i], d, round_up((int)tok, 64), nullptr)) return -1;
                u->region_h[i] = H; u->region_w[i] = W;
                if (u->max_tokens > 77) {       // the region maps of this level (cfgpp_unet_set_regions): sized here, nothing allocated later
                    u->d_region_ids[i] = (unsigned char*)u->dmalloc((size_t)R * round_up((int)tok, 128));
                    CFGPP_REQUIRE(u->d_region_ids[i], "finalize: hipMalloc failed");
                }
                if (u->soft_enabled) {          // the region weights of this level (cfgpp_unet_set_region_weights): sized here as well
                    u->d_region_w[i] = (float*)u->dmalloc((size_t)R * 4 * round_up((int)tok, 128) * sizeof(float));
                    CFGPP_REQUIRE(u->d_region_w[i], "finalize: hipMalloc failed");
                }
            }
            if (i != L - 1) { H /= 2; W /= 2; }
        }
    }
    u->tok_x = (half_t*)u->dmalloc((size_t)R * max_tok_c * 2);
    u->tok_ln = (half_t*)u->dmalloc((size_t)R * max_tok_c * 2);
    u->tok_attn = (half_t*)u->dmalloc((size_t)R * max_tok_c * 2);
    u->tok_ff = (half_t*)u->dmalloc((size_t)R * max_ff * 2);
    u->d_gn_stats = (float*)u->dmalloc((size_t)R * (1024 * 64 * 2 + 64 * 2) * sizeof(float));
    u->d_sin_t = (float*)u->dmalloc((size_t)c0 * sizeof(float));
    u->d_emb_h = (float*)u->dmalloc((size_t)temb_dim * sizeof(float));
    u->d_emb_t = (float*)u->dmalloc((size_t)temb_dim * sizeof(float));
    u->d_emb = (float*)u->dmalloc((size_t)R * temb_dim * sizeof(float));
    CFGPP_REQUIRE(u->tok_x && u->tok_ln && u->tok_attn && u->tok_ff, "finalize: hipMalloc failed");

    // ---- collect every resnet's time_emb_proj into one [sumC][temb] matrix ----
    std::vector<std::string> res_names;
    {
        for (int i = 0; i < L; ++i)
            for (int j = 0; j < c.layers_per_block; ++j) res_names.push_back("down_blocks." + std::to_string(i) + ".resnets." + std::to_string(j));
        res_names.push_back("mid_block.resnets.0"); res_names.push_back("mid_block.resnets.1");
        for (int i = 0; i < L && !u->control; ++i)
            for (int j = 0; j < c.layers_per_block + 1; ++j) res_names.push_back("up_blocks." + std::to_string(i) + ".resnets." + std::to_string(j));
    }
    std::map<std::string, int> temb_off;
    half_t* w_temb_all = nullptr; float* b_temb_all = nullptr;
    {
        std::vector<half_t> wa; std::vector<float> ba; int off = 0;
        for (auto& rn : res_names) {
            HostParam* pw = B.get(rn + ".time_emb_proj.weight"); HostParam* pb = B.get(rn + ".time_emb_proj.bias");
            CFGPP_REQUIRE(pw && pb, "finalize: %s", B.err.c_str());
            temb_off[rn] = off; off += (int)pw->shape[0];
            wa.insert(wa.end(), pw->h.begin(), pw->h.end()); ba.insert(ba.end(), pb->f.begin(), pb->f.end());
            B.drop(rn + ".time_emb_proj.weight"); B.drop(rn + ".time_emb_proj.bias");
        }
        u->temb_total = off;
        w_temb_all = B.upload(wa); b_temb_all = B.upload(ba);
        for (auto& rn : res_names) B.slot(rn + ".time_emb_proj.weight", w_temb_all, SLOT_MEMBER, temb_off[rn]);
        u->d_temb_all = (float*)u->dmalloc((size_t)R * off * sizeof(float));
    }
    const bool per_row_temb = c.addition_embed != 0;
    const int temb_ld = per_row_temb ? u->temb_total : 0;

    // ---- time embedding ops (head of the forward plan) ----
    {
        half_t* w1 = B.linear("time_embedding.linear_1.weight"); float* b1 = B.f32("time_embedding.linear_1.bias");
        half_t* w2 = B.linear("time_embedding.linear_2.weight"); float* b2 = B.f32("time_embedding.linear_2.bias");
        cfgpp_unet* uu = u;
        const float* time_add = nullptr;        // guidance-embedded UNets: linear_1.weight x cond_proj(w_emb), added before the SiLU
        if (u->time_cond) {
            u->w_time1 = w1;
            u->w_cond = B.linear("time_embedding.cond_proj.weight");
            u->d_w_emb = (float*)u->dmalloc((size_t)u->time_cond * sizeof(float));
            u->d_cond_vec = (float*)u->dmalloc((size_t)c0 * sizeof(float));
            u->d_time_add = (float*)u->dmalloc((size_t)temb_dim * sizeof(float));
            CFGPP_REQUIRE(u->w_cond && u->d_w_emb && u->d_cond_vec && u->d_time_add, "finalize: time_embedding.cond_proj: %s",
                          B.ok ? "hipMalloc failed" : B.err.c_str());
            u->h_w_emb.assign((size_t)u->time_cond, 0.f);
            time_add = u->d_time_add;
        }
        u->plan.push_back([=](hipStream_t s, int) { return cfgpp_op_sinusoid(uu->in_t_dev, uu->in_t, uu->d_sin_t, 1, c0, c0, 0, s); });
        u->plan.push_back([=](hipStream_t s, int) { return cfgpp_op_skinny_gemm(uu->d_sin_t, c0, w1, b1, time_add, 0, uu->d_emb_h, temb_dim, 1, temb_dim, c0, 0, 1, s); });
        if (per_row_temb) {
            // emb[r] = linear_2(h) + aug[r or 0]
            u->plan.push_back([=](hipStream_t s, int rows) {
                const int add_ld = uu->ctx_cond_rows == 1 ? 0 : temb_dim;
                return cfgpp_op_skinny_gemm(uu->d_emb_h, 0, w2, b2, uu->d_aug, add_ld, uu->d_emb, temb_dim, rows, temb_dim, temb_dim, 0, 0, s);
            });
            u->plan.push_back([=](hipStream_t s, int rows) {
                return cfgpp_op_skinny_gemm(uu->d_emb, temb_dim, w_temb_all, b_temb_all, nullptr, 0, uu->d_temb_all, uu->temb_total, rows, uu->temb_total, temb_dim, 1, 0, s);
            });
        } else {
            u->plan.push_back([=](hipStream_t s, int) { return cfgpp_op_skinny_gemm(uu->d_emb_h, temb_dim, w2, b2, nullptr, 0, uu->d_emb_t, temb_dim, 1, temb_dim, temb_dim, 0, 0, s); });
            u->plan.push_back([=](hipStream_t s, int) {
                return cfgpp_op_skinny_gemm(uu->d_emb_t, temb_dim, w_temb_all, b_temb_all, nullptr, 0, uu->d_temb_all, uu->temb_total, 1, uu->temb_total, temb_dim, 1, 0, s);
            });
        }
        if (c.addition_embed) {
            const int tdim = c.addition_time_embed_dim, pooled = c.addition_pooled_dim, in = 6 * tdim + pooled;
            half_t* aw1 = B.linear("add_embedding.linear_1.weight"); float* ab1 = B.f32("add_embedding.linear_1.bias");
            half_t* aw2 = B.linear("add_embedding.linear_2.weight"); float* ab2 = B.f32("add_embedding.linear_2.bias");
            u->d_add_in = (float*)u->dmalloc((size_t)R * in * sizeof(float));
            u->d_add_h = (float*)u->dmalloc((size_t)R * temb_dim * sizeof(float));
            u->d_aug = (float*)u->dmalloc((size_t)R * temb_dim * sizeof(float));
            // add_in[r] = [text_embeds[r] | sinusoid(time_ids[r][0..5])]
            u->ctx_plan.push_back([=](hipStream_t s, int) { return cfgpp_op_f16_to_f32_rows(uu->ctx_text, uu->d_add_in, uu->ctx_cond_rows, pooled, in, 0, s); });
            u->ctx_plan.push_back([=](hipStream_t s, int) {
                // 6*cond_rows values, each -> tdim wide, laid out contiguously after the pooled part of its row
                for (int r = 0; r < uu->ctx_cond_rows; ++r) {
                    int e = cfgpp_op_sinusoid(uu->ctx_tids + (long)r * 6, 0.f, uu->d_add_in + (long)r * in + pooled, 6, tdim, tdim, 0, s);
                    if (e) return e;
                }
                return 0;
            });
            u->ctx_plan.push_back([=](hipStream_t s, int) { return cfgpp_op_skinny_gemm(uu->d_add_in, in, aw1, ab1, nullptr, 0, uu->d_add_h, temb_dim, uu->ctx_cond_rows, temb_dim, in, 0, 1, s); });
            u->ctx_plan.push_back([=](hipStream_t s, int) { return cfgpp_op_skinny_gemm(uu->d_add_h, temb_dim, aw2, ab2, nullptr, 0, uu->d_aug, temb_dim, uu->ctx_cond_rows, temb_dim, temb_dim, 0, 0, s); });
        }
    }

    // ---- layer builders ----
    auto load_res = [&](const std::string& p, int cin, int cout) {
        ResW w{}; w.cin = cin; w.cout = cout;
        w.n1g = B.f32(p + ".norm1.weight"); w.n1b = B.f32(p + ".norm1.bias");
        w.w1 = B.conv3(p + ".conv1.weight"); w.b1 = B.f32(p + ".conv1.bias");
        w.n2g = B.f32(p + ".norm2.weight"); w.n2b = B.f32(p + ".norm2.bias");
        w.w2 = B.conv3(p + ".conv2.weight"); w.b2 = B.f32(p + ".conv2.bias");
        if (cin != cout) { w.wsc = B.linear(p + ".conv_shortcut.weight"); w.bsc = B.f32(p + ".conv_shortcut.bias"); }
        w.temb_off = temb_off[p];
        return w;
    };
    // x0 (|| x1) -> new tensor
    auto resblock = [&](const std::string& p, const Tensor& x0, const Tensor* x1, int cout) {
        const int cin = x0.C + (x1 ? x1->C : 0);
        ResW w = load_res(p, cin, cout);
        Tensor g1 = u->acq(x0.H, x0.W, cin);
        P.groupnorm(x0, x1, g1.p, true, w.n1g, w.n1b, 1e-5f, true);
        Tensor h1 = u->acq(x0.H, x0.W, cout);
        P.conv3x3(g1, h1, w.w1, w.b1, 1, u->d_temb_all + w.temb_off, temb_ld, nullptr);
        u->rel(g1);
        Tensor g2 = u->acq(x0.H, x0.W, cout);
        P.groupnorm(h1, nullptr, g2.p, true, w.n2g, w.n2b, 1e-5f, true);
        u->rel(h1);
        Tensor out = u->acq(x0.H, x0.W, cout);
        if (cin != cout) {
            Tensor sc = u->acq(x0.H, x0.W, cout);
            P.conv1x1(x0, x1, sc, w.wsc, w.bsc);
            P.conv3x3(g2, out, w.w2, w.b2, 1, nullptr, 0, &sc);
            u->rel(sc);
        } else {
            P.conv3x3(g2, out, w.w2, w.b2, 1, nullptr, 0, &x0);
        }
        u->rel(g2);
        return out;
    };
    int cross_block_counter = 0;
    long prefix_from = -1;          // >= 0: plan index where the shared CFG prefix starts; the next transformer ends it
    auto transformer = [&](const std::string& p, const Tensor& x, int depth, int nheads, int lvl) {
        half_t* const HQ = u->hq[lvl]; half_t* const HK = u->hk[lvl]; half_t* const HVT = u->hvt[lvl];
        const int C = x.C, tok = x.H * x.W, d = C / nheads, dp = round_up(d, 32);
        const int q_pad = round_up(tok, 128), k_pad = round_up(tok, 64);
        const int ck_pad = std::max(128, round_up(u->max_tokens, 64));
        float* ng = B.f32(p + ".norm.weight"); float* nb = B.f32(p + ".norm.bias");
        half_t* wpi = B.linear(p + ".proj_in.weight"); float* bpi = B.f32(p + ".proj_in.bias");
        half_t* wpo = B.linear(p + ".proj_out.weight"); float* bpo = B.f32(p + ".proj_out.bias");
        P.groupnorm(x, nullptr, u->tok_ln, false, ng, nb, 1e-6f, false);
        P.linear(u->tok_ln, C, u->tok_x, C, wpi, bpi, nullptr, tok);
        for (int k = 0; k < depth; ++k) {
            const std::string b = p + ".transformer_blocks." + std::to_string(k);
            float* l1g = B.f32(b + ".norm1.weight"); float* l1b = B.f32(b + ".norm1.bias");
            float* l2g = B.f32(b + ".norm2.weight"); float* l2b = B.f32(b + ".norm2.bias");
            float* l3g = B.f32(b + ".norm3.weight"); float* l3b = B.f32(b + ".norm3.bias");
            half_t* wqkv = B.concat({b + ".attn1.to_q.weight", b + ".attn1.to_k.weight", b + ".attn1.to_v.weight"});
            half_t* wq2 = B.linear(b + ".attn2.to_q.weight");
            half_t* wff1 = nullptr; float* bff1 = nullptr;
            B.geglu(b + ".ff.net.0.proj", C, &wff1, &bff1);
            half_t* wo1 = B.linear(b + ".attn1.to_out.0.weight"); float* bo1 = B.f32(b + ".attn1.to_out.0.bias");
            half_t* wkv2 = B.concat({b + ".attn2.to_k.weight", b + ".attn2.to_v.weight"});
            half_t* wo2 = B.linear(b + ".attn2.to_out.0.weight"); float* bo2 = B.f32(b + ".attn2.to_out.0.bias");
            half_t* wff2 = B.linear(b + ".ff.net.2.weight"); float* bff2 = B.f32(b + ".ff.net.2.bias");
            // persistent cross-attention K / V^T of this block (filled by set_context)
            half_t* ck = (half_t*)u->dmalloc((size_t)R * nheads * ck_pad * dp * 2);
            half_t* cvt = (half_t*)u->dmalloc((size_t)R * nheads * dp * ck_pad * 2);
            if (!ck || !cvt || cfgpp_op_attention_prepare_vt(cvt, R * nheads, d, ck_pad, nullptr)) { B.ok = false; B.err = "cross-attention K/V^T allocation failed"; }
            {
                cfgpp_unet* uu = u; const int Dc = c.cross_attention_dim; const int ckp = ck_pad;
                IGemmArgs a = base_args(u);
                a.C0 = Dc; a.amode = 0; a.w = wkv2; a.N = 2 * C; a.K = Dc; a.epi = EPI_HEADS;
                a.hq = nullptr; a.hk = ck; a.hvt = cvt; a.part0 = 1; a.part_width = C; a.head_dim = d; a.head_dim_pad = dp;
                a.heads = nheads; a.tok_pad = ckp; a.q_tok_pad = ckp;
                u->ctx_plan.push_back([a, uu](hipStream_t s, int) mutable {
                    IGemmArgs b2 = a; b2.a0 = uu->ctx_ehs; b2.rows_per_batch = uu->ctx_tokens; b2.M = uu->ctx_rows * uu->ctx_tokens;
                    return igemm_launch(b2, s);
                });
            }
            ++cross_block_counter;
            u->ip_ck_pad = ck_pad;
            u->ip_blocks.push_back(cfgpp_unet::IpBlock{b + ".attn2", C, nheads, d, dp, tok, ck, cvt, 0});
            // self-attention
            P.layernorm(u->tok_x, u->tok_ln, l1g, l1b, tok, C);
            P.heads(u->tok_ln, C, wqkv, 3 * C, tok, 0, C, nheads, HQ, HK, HVT, q_pad, k_pad);
            P.attention(HQ, HK, HVT, u->tok_attn, nheads, d, tok, tok, q_pad, k_pad);
            P.linear(u->tok_attn, C, u->tok_x, C, wo1, bo1, u->tok_x, tok);
            // cross-attention
            P.layernorm(u->tok_x, u->tok_ln, l2g, l2b, tok, C);
            P.heads(u->tok_ln, C, wq2, C, tok, 0, C, nheads, HQ, nullptr, nullptr, q_pad, k_pad);
            if (prefix_from >= 0) {
                // end of the shared CFG prefix: the cross-attention below is the first op that sees the text context.  Live from
                // here on: tok_x (residual stream), HQ (its queries) and x (the residual of proj_out), each contiguous in the row.
                u->plan_share.assign(u->plan.size(), 0);
                for (size_t i = (size_t)prefix_from; i < u->plan.size(); ++i) {
                    u->plan_share[i] = 1; ++u->prefix_ops;
                    if (i < u->plan_macs.size()) u->prefix_macs_per_row += u->plan_macs[i];
                }
                half_t* const fp0 = u->tok_x; half_t* const fp1 = HQ; half_t* const fp2 = x.p;
                const long fe0 = (long)tok * C, fe1 = (long)nheads * q_pad * dp, fe2 = (long)(x.H + 2) * (x.W + 2) * C;
                u->plan.push_back([=](hipStream_t s, int h) {
                    if (h <= 0) return 0;                  // a call that does not share
                    half_t* const fp[3] = {fp0, fp1, fp2}; const long fe[3] = {fe0, fe1, fe2};
                    return fanout_rows_launch(fp, fe, 3, h, s);
                });
                u->plan_share.push_back(2);
                u->tag(3, 0.0, "cfg fan-out tok_x + HQ + resid HW=" + std::to_string(tok) + " C=" + std::to_string(C));
                prefix_from = -1;
            }
            {
                cfgpp_unet* uu = u;
                u->attn_macs_per_row += 2.0 * (double)nheads * tok * 77 * d;
                half_t* hq = HQ; half_t* o = u->tok_attn;
                u->plan.push_back([=](hipStream_t s, int rows) {
                    if (uu->regions)        // regional prompts: every query attends to the 77 keys of its region, ONE launch, same launch count
                        return cfgpp_op_attention_region(hq, ck, cvt, o, rows, nheads, d, tok, uu->regions, uu->d_region_ids[lvl],
                                                         uu->region_map_rows == 1 ? 1 : rows, q_pad, ck_pad, s);
                    if (uu->soft_regions)   // soft regional prompts: every query blends the regions' complete softmaxes, ONE launch
                        return cfgpp_op_attention_region_soft(hq, ck, cvt, o, rows, nheads, d, tok, uu->soft_regions, uu->d_region_w[lvl],
                                                              uu->soft_map_rows == 1 ? 1 : rows, q_pad, ck_pad, s);
                    if (uu->ip_active)      // IP-Adapter: text + image keys in ONE launch (head dims padded to 64), same launch count
                        return cfgpp_op_attention_ip(hq, ck, cvt, o, rows, nheads, d, tok, uu->ctx_tokens, uu->ip_n_img, uu->ip_scale, q_pad,
                                                     ck_pad, s);
                    return cfgpp_op_attention_cross(hq, ck, cvt, o, rows, nheads, d, tok, uu->ctx_tokens, q_pad, ck_pad, s);
                });
                u->ip_blocks.back().plan_idx = u->plan.size() - 1;
                u->ip_macs_per_key += 2.0 * (double)nheads * tok * d;
                u->tag(1, 2.0 * (double)nheads * tok * 77 * d, "cross_attn heads=" + std::to_string(nheads) + " N=" + std::to_string(tok) + " d=" + std::to_string(d));
            }
            P.linear(u->tok_attn, C, u->tok_x, C, wo2, bo2, u->tok_x, tok);
            // feed-forward (GEGLU)
            P.layernorm(u->tok_x, u->tok_ln, l3g, l3b, tok, C);
            P.linear(u->tok_ln, C, u->tok_ff, 8 * C, wff1, bff1, nullptr, tok, EPI_GEGLU);
            P.linear(u->tok_ff, 4 * C, u->tok_x, C, wff2, bff2, u->tok_x, tok);
        }
        Tensor out = u->acq(x.H, x.W, C);
        P.linear_to_padded(u->tok_x, C, out, wpo, bpo, x);
        return out;
    };

    // ---- conv_in ----
    int H = c.sample_h, W = c.sample_w;
    Tensor x = u->acq(H, W, c0);
    {
        HostParam* pw = B.get("conv_in.weight"); HostParam* pb = B.get("conv_in.bias");
        CFGPP_REQUIRE(pw && pb, "finalize: %s", B.err.c_str());
        const int Ci = c.in_channels;
        std::vector<float> r((size_t)9 * Ci * c0);
        for (int o = 0; o < c0; ++o) for (int i = 0; i < Ci; ++i) for (int t = 0; t < 9; ++t)
            r[(size_t)(t * Ci + i) * c0 + o] = pw->f[((size_t)o * Ci + i) * 9 + t];
        float* dw = B.upload(r); float* db = B.upload(pb->f);
        cfgpp_unet* uu = u; half_t* xp = x.p; const int HH = H, WW = W;
        if (u->control) {                   // ControlNet: conv_in(z) + the embedded control image (fp16 sum)
            u->d_img_emb = (half_t*)u->dmalloc((size_t)R * (H + 2) * (W + 2) * c0 * sizeof(half_t));
            CFGPP_REQUIRE(u->d_img_emb, "finalize: hipMalloc failed");
            u->plan.push_back([=](hipStream_t s, int rows) {
                return cfgpp_op_conv_in_add(uu->in_z, uu->in_z_half, nullptr, 1, 0, uu->d_img_emb, uu->img_rows, xp, dw, db, rows,
                                            uu->in_z_rows, Ci, HH, WW, c0, s);
            });
        } else if (Ci > c.out_channels) {          // inpaint UNet: latent channels from z, the rest from the condition buffer
            const int Cz = c.out_channels, Cc = Ci - Cz;
            u->d_cond = (half_t*)u->dmalloc((size_t)R * Cc * H * W * sizeof(half_t));
            CFGPP_REQUIRE(u->d_cond, "finalize: hipMalloc failed");
            u->plan.push_back([=](hipStream_t s, int rows) {
                return cfgpp_op_conv_in_cond(uu->in_z, uu->in_z_half, uu->d_cond, uu->cond_rows, Cc, xp, dw, db, rows, uu->in_z_rows, Cz,
                                             HH, WW, c0, s);
            });
        } else {
            u->plan.push_back([=](hipStream_t s, int rows) {
                return cfgpp_op_conv_in(uu->in_z, uu->in_z_half, xp, dw, db, rows, uu->in_z_rows, Ci, HH, WW, c0, s);
            });
        }
    }
    std::vector<Tensor> skips; skips.push_back(x);
    // ---- down ----
    for (int i = 0; i < L; ++i) {
        const int co = c.block_out_channels[i];
        const std::string p = "down_blocks." + std::to_string(i);
        for (int j = 0; j < c.layers_per_block; ++j) {
            if (i == 0 && j == 0 && !per_row_temb && c.level_has_attn[0]) prefix_from = (long)u->plan.size();
            Tensor y = resblock(p + ".resnets." + std::to_string(j), x, nullptr, co);
            if (c.level_has_attn[i]) {
                Tensor z = transformer(p + ".attentions." + std::to_string(j), y, c.transformer_depth[i], c.num_heads[i], i);
                u->rel(y); y = z;
            }
            x = y; skips.push_back(x);
        }
        if (i != L - 1) {
            half_t* wd = B.conv3(p + ".downsamplers.0.conv.weight"); float* bd = B.f32(p + ".downsamplers.0.conv.bias");
            H /= 2; W /= 2;
            Tensor y = u->acq(H, W, co);
            P.conv3x3(x, y, wd, bd, 2, nullptr, 0, nullptr);
            x = y; skips.push_back(x);
        }
    }
    // ---- mid ----
    {
        const int cm = c.block_out_channels[L - 1];
        Tensor y = resblock("mid_block.resnets.0", x, nullptr, cm);          // x is also the last skip: keep it
        Tensor z = transformer("mid_block.attentions.0", y, c.transformer_depth[L - 1], c.num_heads[L - 1], L - 1);
        u->rel(y);
        Tensor w = resblock("mid_block.resnets.1", z, nullptr, cm);
        u->rel(z);
        x = w;
    }
    if (u->control) {
        int e = controlnet_tail(u, B, P, skips, x);
        if (e) return e;
        skips.clear();
        CFGPP_REQUIRE(B.ok, "finalize: %s", B.err.c_str());
        CFGPP_HIP_CHECK(hipDeviceSynchronize());
        u->plan_kind.resize(u->plan.size(), 3); u->plan_macs.resize(u->plan.size(), 0.0); u->plan_desc.resize(u->plan.size());
        u->plan_share.resize(u->plan.size(), 0);
        u->finalized = true;
        return 0;
    }
    // ---- ControlNet residuals (cfgpp_unet_attach_control): skip_i += down_res[i], mid += mid_res, after the mid block has read
    // the last skip.  The up path's GroupNorms must not use the statistics the skips' producers wrote: the op clears their flags.
    {
        u->ctrl_dst = skips; u->ctrl_dst.push_back(x);
        u->d_ctrl_tab = (CnAddEntry*)u->dmalloc(u->ctrl_dst.size() * sizeof(CnAddEntry));
        CFGPP_REQUIRE(u->d_ctrl_tab, "finalize: hipMalloc failed");
        for (const Tensor& t : u->ctrl_dst) u->ctrl_max_n8 = std::max(u->ctrl_max_n8, (long)R * t.H * t.W * (t.C / 8));
        cfgpp_unet* uu = u;
        const int n = (int)u->ctrl_dst.size();
        u->plan.push_back([uu, n](hipStream_t s, int rows) {
            if (!uu->ctrl || uu->ctrl_scale == 0.f) return 0;
            for (const Tensor& t : uu->ctrl_dst) if (t.gst_ok) *t.gst_ok = 0;
            return cn_residual_add_launch(uu->d_ctrl_tab, n, uu->ctrl_max_n8, rows, uu->ctrl_scale, s);
        });
        u->tag(3, 0.0, "controlnet residual add");
    }
    // ---- up ----
    for (int i = 0; i < L; ++i) {
        const int lvl = L - 1 - i;
        const int co = c.block_out_channels[lvl];
        const std::string p = "up_blocks." + std::to_string(i);
        for (int j = 0; j < c.layers_per_block + 1; ++j) {
            Tensor skip = skips.back(); skips.pop_back();
            if (i < 2) {
                // FreeU (cfgpp_unet_set_freeu): x[:, :C / 2] *= b_i and the low-pass of `skip` scaled by s_i, IN PLACE, before the
                // resnet that concatenates the two.  In place is safe: x is read only by this resblock's GroupNorm and 1x1
                // shortcut and released right after it; `skip` is read only there too - the one skip the mid block also reads (its
                // input) was read before the up path starts; the ControlNet residual add precedes the up path (diffusers adds the
                // residuals to the skips first, then runs the up blocks); tune_plan and cfgpp_unet_profile re-run WHOLE forwards,
                // which write both tensors again.  The statistics their producers left (Tensor::gst) describe the unedited values:
                // where a tensor really changes (scale != 1) its flag is cleared, as the residual add does, and the GroupNorm
                // takes its own.  plan_share 3: the op is part of a call only while FreeU is on (EngineBase::rows_for).
                if (!u->d_freeu_tw[i]) {
                    std::vector<float> tw((size_t)2 * x.H + 2 * x.W);
                    freeu_twiddles(x.H, x.W, tw.data());
                    u->d_freeu_tw[i] = B.upload(tw);
                }
                cfgpp_unet* uu = u;
                const Tensor hx = x, sk = skip; const float* tw = u->d_freeu_tw[i]; const int blk = i;
                u->plan.push_back([uu, hx, sk, tw, blk](hipStream_t s, int rows) {
                    if (rows <= 0 || !uu->freeu_on) return 0;
                    const float fb = uu->freeu_b[blk], fs = uu->freeu_s[blk];
                    if (fb != 1.f && hx.gst_ok) *hx.gst_ok = 0;
                    if (fs != 1.f && sk.gst_ok) *sk.gst_ok = 0;
                    return freeu_launch(hx.p, hx.C, sk.p, sk.C, rows, hx.H, hx.W, fb, fs, tw, s);
                });
                u->tag(3, 0.0, "freeu " + p + ".resnets." + std::to_string(j));
                u->plan_share.resize(u->plan.size(), 0); u->plan_share.back() = 3;
            }
            Tensor y = resblock(p + ".resnets." + std::to_string(j), x, &skip, co);
            u->rel(x); u->rel(skip);
            if (c.level_has_attn[lvl]) {
                Tensor z = transformer(p + ".attentions." + std::to_string(j), y, c.transformer_depth[lvl], c.num_heads[lvl], lvl);
                u->rel(y); y = z;
            }
            x = y;
        }
        if (i != L - 1) {
            half_t* wu = B.conv3(p + ".upsamplers.0.conv.weight"); float* bu = B.f32(p + ".upsamplers.0.conv.bias");
            H *= 2; W *= 2;
            Tensor y = u->acq(H, W, co);
            P.conv3x3(x, y, wu, bu, 3, nullptr, 0, nullptr);
            u->rel(x); x = y;
        }
    }
    // ---- out ----
    {
        float* g = B.f32("conv_norm_out.weight"); float* b = B.f32("conv_norm_out.bias");
        Tensor gn = u->acq(H, W, c0);
        P.groupnorm(x, nullptr, gn.p, true, g, b, 1e-5f, true);
        HostParam* pw = B.get("conv_out.weight"); float* bo = B.f32("conv_out.bias");
        CFGPP_REQUIRE(pw, "finalize: %s", B.err.c_str());
        const int Co = c.out_channels;
        CFGPP_REQUIRE(Co <= 4, "finalize: out_channels %d > 4 unsupported", Co);
        std::vector<half_t> r((size_t)Co * 9 * c0);
        for (int o = 0; o < Co; ++o) for (int i = 0; i < c0; ++i) for (int t = 0; t < 9; ++t)
            r[((size_t)o * 9 + t) * c0 + i] = pw->h[((size_t)o * c0 + i) * 9 + t];
        half_t* dw = B.upload(r);
        cfgpp_unet* uu = u; half_t* gp = gn.p; const int HH = H, WW = W;
        u->macs_per_row += (double)H * W * Co * 9.0 * c0 + (double)c.sample_h * c.sample_w * c0 * 9.0 * c.in_channels;
        u->plan.push_back([=](hipStream_t s, int rows) { return cfgpp_op_conv_out(gp, uu->out_eps, 1, dw, bo, rows, HH, WW, c0, Co, s); });
    }
    CFGPP_REQUIRE(B.ok, "finalize: %s", B.err.c_str());
    CFGPP_REQUIRE(skips.empty(), "finalize: internal error, %d skips left", (int)skips.size());
    CFGPP_HIP_CHECK(hipDeviceSynchronize());
    u->plan_kind.resize(u->plan.size(), 3); u->plan_macs.resize(u->plan.size(), 0.0); u->plan_desc.resize(u->plan.size());
    u->plan_share.resize(u->plan.size(), 0);
    u->finalized = true;
    return 0;
}

int cfgpp_unet_set_context(cfgpp_unet* u, const void* ehs, int rows, int tokens, const void* text_embeds,
                           const void* time_ids, int cond_rows, void* stream) {
    CFGPP_REQUIRE(u && u->finalized, "set_context: context not finalized");
    CFGPP_REQUIRE(ehs && rows > 0 && rows <= u->cfg.max_rows, "set_context: rows=%d (max %d)", rows, u->cfg.max_rows);
    CFGPP_REQUIRE(tokens >= 77 && tokens % 77 == 0 && tokens <= u->max_tokens,
                  "set_context: tokens=%d (a multiple of 77 up to max_tokens=%d, which cfgpp_unet_set_max_tokens raises before finalize)", tokens,
                  u->max_tokens);
    if (u->cfg.addition_embed) {
        CFGPP_REQUIRE(text_embeds && time_ids, "set_context: SDXL needs text_embeds and time_ids");
        CFGPP_REQUIRE(cond_rows == rows || cond_rows == 1, "set_context: cond_rows=%d must be rows (%d) or 1", cond_rows, rows);
    }
    u->ctx_ehs = (const half_t*)ehs; u->ctx_rows = rows; u->ctx_tokens = tokens;
    u->ctx_text = (const half_t*)text_embeds; u->ctx_tids = (const float*)time_ids; u->ctx_cond_rows = cond_rows;
    for (auto& op : u->ctx_plan) { int e = op((hipStream_t)stream, rows); if (e) return e; }
    u->ctx_set = true;
    u->retag_cross();
    return 0;
}

int cfgpp_unet_set_max_tokens(cfgpp_unet* u, int max_tokens) {
    CFGPP_REQUIRE(u, "set_max_tokens: null engine");
    CFGPP_REQUIRE(!u->finalized, "set_max_tokens: max_tokens=%d after cfgpp_unet_finalize (the cross-attention buffers are sized there)", max_tokens);
    CFGPP_REQUIRE(max_tokens == 77 || max_tokens == 154 || max_tokens == 231 || max_tokens == 308,
                  "set_max_tokens: max_tokens=%d (77, 154, 231 or 308)", max_tokens);
    u->max_tokens = max_tokens;
    return 0;
}

// Regional prompts (include/cfgpp_regions.h).  The level maps are nearest downsamples of the level-0 map, id_l[y][x] = id_0[y << l][x << l]
// (what F.interpolate(mode="nearest") gives for these integer factors), made on the host and copied into the buffers finalize sized.
int cfgpp_unet_set_regions(cfgpp_unet* u, const unsigned char* ids_host, int map_rows, int n_regions) {
    CFGPP_REQUIRE(u && u->finalized, "set_regions: the engine is not finalized");
    if (!ids_host && map_rows == 0 && n_regions == 0) {        // off: the plain engine
        if (u->regions) { u->regions = 0; u->region_map_rows = 0; u->retag_cross(); }
        return 0;
    }
    CFGPP_REQUIRE(!u->control, "set_regions: a ControlNet-mode engine takes no regional prompts (regions with ControlNet are not built)");
    CFGPP_REQUIRE(u->ip_kind == cfgpp_unet::IP_NONE && !u->ip_active, "set_regions: an IP-Adapter is loaded (regions with an IP-Adapter are not built: "
                  "its image slots sit at key 96 of the text buffers)");
    CFGPP_REQUIRE(n_regions >= 2 && n_regions <= 4, "set_regions: n_regions=%d (2 .. 4; (NULL, 0, 0) turns regions off)", n_regions);
    CFGPP_REQUIRE(ids_host, "set_regions: null region map");
    CFGPP_REQUIRE(u->max_tokens >= 77 * n_regions, "set_regions: n_regions=%d needs max_tokens >= %d, the engine was built with max_tokens=%d "
                  "(cfgpp_unet_set_max_tokens before finalize)", n_regions, 77 * n_regions, u->max_tokens);
    CFGPP_REQUIRE(map_rows == 1 || (map_rows >= 1 && map_rows <= u->cfg.max_rows && (!u->ctx_set || map_rows == u->ctx_rows)),
                  "set_regions: map_rows=%d (1, or the context's row count %d)", map_rows, u->ctx_set ? u->ctx_rows : u->cfg.max_rows);
    const int H0 = u->cfg.sample_h, W0 = u->cfg.sample_w;
    for (long i = 0; i < (long)map_rows * H0 * W0; ++i)
        if (ids_host[i] >= n_regions) {
            cfgpp_set_error("set_regions: region id %d at row %ld, pixel (%ld, %ld) but n_regions=%d (ids are 0 .. n_regions - 1)", (int)ids_host[i],
                            i / ((long)H0 * W0), (i / W0) % H0, i % W0, n_regions);
            return -2;
        }
    CFGPP_HIP_CHECK(hipSetDevice(u->device));
    CFGPP_HIP_CHECK(hipDeviceSynchronize());                   // no forward in flight reads the maps that are rewritten below
    std::vector<unsigned char> lvl_map;
    for (int l = 0; l < u->cfg.num_levels; ++l) {
        if (!u->d_region_ids[l]) continue;
        const int h = u->region_h[l], w = u->region_w[l], q_pad = round_up(h * w, 128);
        const int fy = H0 / h, fx = W0 / w;
        lvl_map.assign((size_t)map_rows * q_pad, 0);
        for (int r = 0; r < map_rows; ++r)
            for (int y = 0; y < h; ++y)
                for (int x = 0; x < w; ++x)
                    lvl_map[(size_t)r * q_pad + y * w + x] = ids_host[((size_t)r * H0 + (size_t)y * fy) * W0 + (size_t)x * fx];
        CFGPP_HIP_CHECK(hipMemcpy(u->d_region_ids[l], lvl_map.data(), lvl_map.size(), hipMemcpyHostToDevice));
    }
    u->regions = n_regions; u->region_map_rows = map_rows;
    u->soft_regions = 0; u->soft_map_rows = 0;                 // exclusive with the soft weights (include/cfgpp_regions_soft.h)
    u->retag_cross();
    return 0;
}

// Soft regional prompts (include/cfgpp_regions_soft.h)
int cfgpp_unet_enable_region_weights(cfgpp_unet* u) {
    CFGPP_REQUIRE(u, "enable_region_weights: null engine");
    CFGPP_REQUIRE(!u->finalized, "enable_region_weights: after cfgpp_unet_finalize (the per-level weight buffers are allocated there)");
    CFGPP_REQUIRE(u->max_tokens > 77, "enable_region_weights: max_tokens=%d (regions need max_tokens > 77: cfgpp_unet_set_max_tokens first)", u->max_tokens);
    u->soft_enabled = true;
    return 0;
}

// The level weights are nearest downsamples of the level-0 weights, w_l[r][y][x] = w_0[r][y << l][x << l], made on the host and copied
// into the buffers finalize sized.
int cfgpp_unet_set_region_weights(cfgpp_unet* u, const float* w_host, int map_rows, int n_regions) {
    CFGPP_REQUIRE(u && u->finalized, "set_region_weights: the engine is not finalized");
    if (!w_host && map_rows == 0 && n_regions == 0) {          // off
        if (u->soft_regions) { u->soft_regions = 0; u->soft_map_rows = 0; u->retag_cross(); }
        return 0;
    }
    CFGPP_REQUIRE(!u->control, "set_region_weights: a ControlNet-mode engine takes no regional prompts (regions with ControlNet are not built)");
    CFGPP_REQUIRE(u->ip_kind == cfgpp_unet::IP_NONE && !u->ip_active, "set_region_weights: an IP-Adapter is loaded (regions with an IP-Adapter are not "
                  "built: its image slots sit at key 96 of the text buffers)");
    CFGPP_REQUIRE(u->soft_enabled, "set_region_weights: the engine was not enabled for region weights (cfgpp_unet_enable_region_weights before finalize)");
    CFGPP_REQUIRE(n_regions >= 2 && n_regions <= 4, "set_region_weights: n_regions=%d (2 .. 4; (NULL, 0, 0) turns the weights off)", n_regions);
    CFGPP_REQUIRE(w_host, "set_region_weights: null weights");
    CFGPP_REQUIRE(u->max_tokens >= 77 * n_regions, "set_region_weights: n_regions=%d needs max_tokens >= %d, the engine was built with max_tokens=%d "
                  "(cfgpp_unet_set_max_tokens before finalize)", n_regions, 77 * n_regions, u->max_tokens);
    CFGPP_REQUIRE(map_rows == 1 || (map_rows >= 1 && map_rows <= u->cfg.max_rows && (!u->ctx_set || map_rows == u->ctx_rows)),
                  "set_region_weights: map_rows=%d (1, or the context's row count %d)", map_rows, u->ctx_set ? u->ctx_rows : u->cfg.max_rows);
    const int H0 = u->cfg.sample_h, W0 = u->cfg.sample_w;
    const long HW = (long)H0 * W0;
    for (long r = 0; r < map_rows; ++r)
        for (long p = 0; p < HW; ++p) {
            float sum = 0.f;
            for (int g = 0; g < n_regions; ++g) {
                const float v = w_host[(r * n_regions + g) * HW + p];
                if (!(v >= 0.f) || !std::isfinite(v)) {
                    cfgpp_set_error("set_region_weights: weight %g at row %ld, region %d, pixel (%ld, %ld) (weights are finite and >= 0)", (double)v, r, g,
                                    p / W0, p % W0);
                    return -2;
                }
                sum += v;
            }
            if (!(std::fabs(sum - 1.f) <= 1e-4f)) {
                cfgpp_set_error("set_region_weights: the weights at row %ld, pixel (%ld, %ld) sum to %.7g (1 +- 1e-4)", r, p / W0, p % W0, (double)sum);
                return -2;
            }
        }
    CFGPP_HIP_CHECK(hipSetDevice(u->device));
    CFGPP_HIP_CHECK(hipDeviceSynchronize());                   // no forward in flight reads the weights that are rewritten below
    std::vector<float> lvl_w;
    for (int l = 0; l < u->cfg.num_levels; ++l) {
        if (!u->d_region_w[l]) continue;
        const int h = u->region_h[l], w = u->region_w[l], q_pad = round_up(h * w, 128);
        const int fy = H0 / h, fx = W0 / w;
        lvl_w.assign((size_t)map_rows * n_regions * q_pad, 0.f);
        for (int r = 0; r < map_rows; ++r)
            for (int g = 0; g < n_regions; ++g)
                for (int y = 0; y < h; ++y)
                    for (int x = 0; x < w; ++x)
                        lvl_w[((size_t)r * n_regions + g) * q_pad + y * w + x] = w_host[(((size_t)r * n_regions + g) * H0 + (size_t)y * fy) * W0 + (size_t)x * fx];
        CFGPP_HIP_CHECK(hipMemcpy(u->d_region_w[l], lvl_w.data(), lvl_w.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    u->regions = 0; u->region_map_rows = 0;                    // exclusive with the hard id map
    u->soft_regions = n_regions; u->soft_map_rows = map_rows;
    u->retag_cross();
    return 0;
}

// what a forward / profile needs of the regional state (by name, with both numbers)
static int regions_ready(const cfgpp_unet* u, int rows, const char* who) {
    if (u->soft_regions) {
        if (u->ctx_tokens != 77 * u->soft_regions) {
            cfgpp_set_error("%s: region weights are on with n_regions=%d (a context of %d tokens) but the context has tokens=%d", who, u->soft_regions,
                            77 * u->soft_regions, u->ctx_tokens);
            return -2;
        }
        if (u->soft_map_rows != 1 && u->soft_map_rows != rows) {
            cfgpp_set_error("%s: the region weights were set for map_rows=%d, the call runs rows=%d (1 or rows)", who, u->soft_map_rows, rows);
            return -2;
        }
        return 0;
    }
    if (!u->regions) return 0;
    if (u->ctx_tokens != 77 * u->regions) {
        cfgpp_set_error("%s: regions are on with n_regions=%d (a context of %d tokens) but the context has tokens=%d", who, u->regions, 77 * u->regions,
                        u->ctx_tokens);
        return -2;
    }
    if (u->region_map_rows != 1 && u->region_map_rows != rows) {
        cfgpp_set_error("%s: the region map was set for map_rows=%d, the call runs rows=%d (1 or rows)", who, u->region_map_rows, rows);
        return -2;
    }
    return 0;
}

// guidance-embedded UNets (LCM distillations; include/cfgpp_lcm.h): the extra parameter time_embedding.cond_proj.weight [c0][dim]
int cfgpp_unet_set_time_cond(cfgpp_unet* u, int dim) {
    CFGPP_REQUIRE(u, "set_time_cond: null engine");
    CFGPP_REQUIRE(!u->finalized, "set_time_cond: time_cond_proj_dim=%d after cfgpp_unet_finalize (the parameter table is fixed there)", dim);
    CFGPP_REQUIRE(!u->control, "set_time_cond: a ControlNet-mode engine (out_channels = 0) has no guidance embedding");
    CFGPP_REQUIRE(u->time_cond == 0, "set_time_cond: already set (time_cond_proj_dim=%d)", u->time_cond);
    CFGPP_REQUIRE(dim >= 8 && dim % 8 == 0 && dim <= 4096, "set_time_cond: time_cond_proj_dim=%d (a multiple of 8 in 8 .. 4096)", dim);
    expect_linear(u, "time_embedding.cond_proj", u->cfg.block_out_channels[0], dim, false);
    u->time_cond = dim;
    return 0;
}

// once per job: d_time_add = linear_1.weight x (cond_proj.weight x w_emb), two skinny-GEMM launches on `stream`
int cfgpp_unet_guidance_embedding(cfgpp_unet* u, const float* w_emb_host, void* stream) {
    CFGPP_REQUIRE(u && u->finalized, "guidance_embedding: the engine is not finalized");
    CFGPP_REQUIRE(u->time_cond > 0, "guidance_embedding: this UNet has no time_embedding.cond_proj (cfgpp_unet_set_time_cond before finalize)");
    CFGPP_REQUIRE(w_emb_host, "guidance_embedding: null embedding");
    const int dim = u->time_cond, c0 = u->cfg.block_out_channels[0], temb_dim = 4 * c0;
    for (int i = 0; i < dim; ++i) CFGPP_REQUIRE(std::isfinite(w_emb_host[i]), "guidance_embedding: w_emb[%d] is not finite", i);
    hipStream_t s = (hipStream_t)stream;
    std::memcpy(u->h_w_emb.data(), w_emb_host, (size_t)dim * sizeof(float));
    CFGPP_HIP_CHECK(hipMemcpyAsync(u->d_w_emb, u->h_w_emb.data(), (size_t)dim * sizeof(float), hipMemcpyHostToDevice, s));
    int e = cfgpp_op_skinny_gemm(u->d_w_emb, dim, u->w_cond, nullptr, nullptr, 0, u->d_cond_vec, c0, 1, c0, dim, 0, 0, s);
    if (e) return e;
    e = cfgpp_op_skinny_gemm(u->d_cond_vec, c0, u->w_time1, nullptr, nullptr, 0, u->d_time_add, temb_dim, 1, temb_dim, c0, 0, 0, s);
    if (e) return e;
    u->time_cond_set = true;
    return 0;
}

// diffusers UNet2DConditionModel.enable_freeu / disable_freeu; the edits themselves are the plan ops in front of the resnets of
// up_blocks.0 / up_blocks.1 (finalize).  Host state only: the next forward reads it, a graph capture bakes it in (GraphKey).
int cfgpp_unet_set_freeu(cfgpp_unet* u, float s1, float s2, float b1, float b2, int enable) {
    CFGPP_REQUIRE(u && u->finalized, "set_freeu: the engine is not finalized");
    CFGPP_REQUIRE(!u->control, "set_freeu: a ControlNet-mode engine (out_channels = 0) has no up path: FreeU applies to the UNet it is attached to");
    if (!enable) { u->freeu_on = false; return 0; }
    CFGPP_REQUIRE(std::isfinite(s1) && std::isfinite(s2) && std::isfinite(b1) && std::isfinite(b2),
                  "set_freeu: non-finite value (s1=%f s2=%f b1=%f b2=%f)", (double)s1, (double)s2, (double)b1, (double)b2);
    const int hmin = u->cfg.sample_h >> (u->cfg.num_levels - 1), wmin = u->cfg.sample_w >> (u->cfg.num_levels - 1);
    CFGPP_REQUIRE(hmin >= 2 && wmin >= 2, "set_freeu: up_blocks.0 runs on %d x %d planes (the low-pass needs at least 2 x 2)", hmin, wmin);
    u->freeu_s[0] = s1; u->freeu_s[1] = s2; u->freeu_b[0] = b1; u->freeu_b[1] = b2;
    u->freeu_on = true;
    return 0;
}

int cfgpp_unet_image_condition(cfgpp_unet* u, const void* cond, int cond_rows, void* stream) {
    CFGPP_REQUIRE(u && u->finalized, "image_condition: engine not finalized");
    if (u->control) {           // ControlNet: embed the control image once per job (ControlNetConditioningEmbedding)
        CFGPP_REQUIRE(cond && cond_rows > 0 && cond_rows <= u->cfg.max_rows, "image_condition: ControlNet image_rows=%d (1 .. %d)", cond_rows,
                      u->cfg.max_rows);
        u->img_in = cond; u->img_in_half = 1;
        for (auto& op : u->img_plan) { int e = op((hipStream_t)stream, cond_rows); if (e) return e; }
        u->img_in = nullptr;
        u->img_rows = cond_rows;
        return 0;
    }
    CFGPP_REQUIRE(u->cfg.in_channels > u->cfg.out_channels && u->d_cond,
                  "image_condition: this UNet takes %d input channels for %d latent channels - no image condition (not an inpaint UNet)",
                  u->cfg.in_channels, u->cfg.out_channels);
    CFGPP_REQUIRE(cond && cond_rows > 0 && cond_rows <= u->cfg.max_rows, "image_condition: cond_rows=%d (1 .. %d)", cond_rows, u->cfg.max_rows);
    const size_t bytes = (size_t)cond_rows * (u->cfg.in_channels - u->cfg.out_channels) * u->cfg.sample_h * u->cfg.sample_w * sizeof(half_t);
    CFGPP_HIP_CHECK(hipMemcpyAsync(u->d_cond, cond, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    u->cond_rows = cond_rows;
    return 0;
}

// ---- IP-Adapter ------------------------------------------------------------------------------------------------------------
// diffusers `load_ip_adapter` for the non-"plus" adapters (ip-adapter_sd15, ip-adapter_sdxl, ip-adapter_sdxl_vit-h):
// `unet.encoder_hid_proj` = ImageProjection (Linear embed_dim -> n_img * cross_dim, reshape, LayerNorm) and one
// IPAdapterAttnProcessor2_0 per cross-attention with its own to_k_ip / to_v_ip.  No reference counterpart.
static int ip_fail(const char* key, const char* why) { cfgpp_set_error("ip_load: %s: %s", key, why); return -2; }

// The Resampler's tensors (include/cfgpp_ip_plus.h) by their published names under "image_proj." and what each axis is: a vector
// has cdim -1; matrices are [rdim][cdim].  (latents [1, n_q, D]: the leading axes are taken off before the table is consulted.)
enum { RK_D, RK_E, RK_INNER, RK_2INNER, RK_FF, RK_CROSS };
struct ResSpec { const char* name; int rdim, cdim; };
static const ResSpec RES_GLOBAL[cfgpp_unet::RG_COUNT] = {
    {"latents", RK_D, -1}, {"proj_in.weight", RK_D, RK_E}, {"proj_in.bias", RK_D, -1}, {"proj_out.weight", RK_CROSS, RK_D},
    {"proj_out.bias", RK_CROSS, -1}, {"norm_out.weight", RK_CROSS, -1}, {"norm_out.bias", RK_CROSS, -1}};
static const ResSpec RES_LAYER[cfgpp_unet::RL_COUNT] = {
    {"0.norm1.weight", RK_D, -1}, {"0.norm1.bias", RK_D, -1}, {"0.norm2.weight", RK_D, -1}, {"0.norm2.bias", RK_D, -1},
    {"0.to_q.weight", RK_INNER, RK_D}, {"0.to_kv.weight", RK_2INNER, RK_D}, {"0.to_out.weight", RK_D, RK_INNER},
    {"1.0.weight", RK_D, -1}, {"1.0.bias", RK_D, -1}, {"1.1.weight", RK_FF, RK_D}, {"1.3.weight", RK_D, RK_FF}};
// "image_proj.<global>" -> (layer -1, slot); "image_proj.layers.<i>.<tail>" -> (i, slot), i unchecked
static bool res_parse_key(const std::string& k, int& layer, int& slot) {
    const std::string pre = "image_proj.";
    if (k.compare(0, pre.size(), pre) != 0) return false;
    const std::string rest = k.substr(pre.size());
    for (int i = 0; i < cfgpp_unet::RG_COUNT; ++i)
        if (rest == RES_GLOBAL[i].name) { layer = -1; slot = i; return true; }
    if (rest.compare(0, 7, "layers.") != 0) return false;
    size_t p = 7; long idx = 0;
    while (p < rest.size() && rest[p] >= '0' && rest[p] <= '9' && p < 7 + 6) idx = idx * 10 + (rest[p++] - '0');
    if (p == 7 || p >= rest.size() || rest[p] != '.') return false;
    const std::string tail = rest.substr(p + 1);
    for (int i = 0; i < cfgpp_unet::RL_COUNT; ++i)
        if (tail == RES_LAYER[i].name) { layer = (int)idx; slot = i; return true; }
    return false;
}

int cfgpp_unet_ip_load(cfgpp_unet* u, const char* key, const void* host, int dtype, const long* shape, int ndim) {
    CFGPP_REQUIRE(u && u->finalized, "ip_load: the engine is not finalized (the adapter attaches to the uploaded UNet)");
    CFGPP_REQUIRE(!u->control, "ip_load: a ControlNet takes no image tokens (diffusers passes it the text context only)");
    CFGPP_REQUIRE(!key || u->max_tokens == 77, "ip_load: IP-Adapter on an engine with max_tokens=%d (the image slots sit at key 96 of a 128-slot "
                  "buffer: max_tokens must be 77)", u->max_tokens);
    CFGPP_HIP_CHECK(hipSetDevice(u->device));
    if (!key) {                 // drop the adapter
        CFGPP_HIP_CHECK(hipDeviceSynchronize());        // an earlier forward may still read its K / V^T slots
        u->ip_drop();
        for (const auto& b : u->ip_blocks)
            if (cfgpp_op_attention_clear_slots(b.ck, b.cvt, u->max_rows * b.nheads, b.d, u->ip_ck_pad, cfgpp_unet::IP_SLOT, cfgpp_unet::IP_MAX, nullptr)) return -1;
        return 0;
    }
    CFGPP_REQUIRE(host && shape && (dtype == 0 || dtype == 1), "ip_load: %s: null tensor or dtype %d (0 fp32, 1 fp16)", key, dtype);
    const std::string k = key;
    const long cross = u->cfg.cross_attention_dim;
    long n = 1; for (int i = 0; i < ndim; ++i) n *= shape[i];
    auto to_half = [&](std::vector<half_t>& h) {
        h.resize(n);
        if (dtype == 0) { const float* s = (const float*)host; for (long i = 0; i < n; ++i) h[i] = (half_t)s[i]; }
        else std::memcpy(h.data(), host, n * sizeof(half_t));
    };
    auto to_float = [&](std::vector<float>& f) {
        f.resize(n);
        if (dtype == 0) std::memcpy(f.data(), host, n * sizeof(float));
        else { const half_t* s = (const half_t*)host; for (long i = 0; i < n; ++i) f[i] = (float)s[i]; }
    };
    // a tensor that replaces an earlier one is uploaded first and swapped in after: a failed call changes nothing
    auto put = [&](void** slot, const void* data, size_t bytes) {
        void* d = u->ip_malloc(bytes);
        if (!d) return ip_fail(key, "out of device memory");
        if (hipMemcpy(d, data, bytes, hipMemcpyHostToDevice) != hipSuccess) { u->ip_free(d); return ip_fail(key, "hipMemcpy failed"); }
        if (*slot) { hipDeviceSynchronize(); u->ip_free(*slot); }
        *slot = d;
        return 0;
    };
    auto changed = [&]() { if (u->ip_active) u->ip_set_active(false, 0, 0.f); u->ip_src = nullptr; };      // the slots are stale now
    // an adapter has ONE image projection: the first image_proj.* tensor after a drop fixes the kind
    const bool linear_key = k == "image_proj.proj.weight" || k == "image_proj.proj.bias" || k == "image_proj.norm.weight" || k == "image_proj.norm.bias";
    int res_layer = -1, res_slot = -1;
    const bool res_key = res_parse_key(k, res_layer, res_slot);
    if ((linear_key && u->ip_kind == cfgpp_unet::IP_RESAMPLER) || (res_key && u->ip_kind == cfgpp_unet::IP_LINEAR)) {
        cfgpp_set_error("ip_load: %s: a tensor of the %s image projection, but this adapter's first image_proj tensor made it a %s adapter: drop it "
                        "(key == NULL) first", key, linear_key ? "Linear + LayerNorm" : "Resampler (\"plus\")", linear_key ? "Resampler (\"plus\")" : "Linear + LayerNorm");
        return -2;
    }
    if (res_key && res_layer >= cfgpp_unet::RES_MAX_DEPTH) {
        cfgpp_set_error("ip_load: %s: layer %d, the Resampler may have 1 .. %d layers", key, res_layer, cfgpp_unet::RES_MAX_DEPTH);
        return -2;
    }
    if (res_key) {
        // Resampler tensor: its shape must fit the UNet and the geometry the tensors loaded so far fixed (every layer has layer 0's shapes)
        const ResSpec& sp = res_layer < 0 ? RES_GLOBAL[res_slot] : RES_LAYER[res_slot];
        cfgpp_unet::Resampler g = u->res;           // the geometry with this tensor, committed after the upload
        long dim[2] = {0, 0}; int nd = ndim;
        const long* sh = shape;
        if (res_layer < 0 && res_slot == cfgpp_unet::RG_LATENTS) {
            if (ndim == 3 && shape[0] == 1) { sh = shape + 1; nd = 2; }
            if (nd != 2 || sh[0] < 1 || sh[0] > cfgpp_unet::IP_MAX) {
                cfgpp_set_error("ip_load: %s: shape [%ld, %ld, %ld], expected [1, n_q, D] with 1 <= n_q <= %d image tokens", key, ndim > 0 ? shape[0] : 0,
                                ndim > 1 ? shape[1] : 0, ndim > 2 ? shape[2] : 0, cfgpp_unet::IP_MAX);
                return -2;
            }
            if (g.nq && g.nq != sh[0]) { cfgpp_set_error("ip_load: %s: n_q %ld, the latents loaded before have %d", key, sh[0], g.nq); return -2; }
            g.nq = (int)sh[0]; sh += 1; nd = 1;      // the remaining axis is D
        }
        if (nd != (sp.cdim >= 0 ? 2 : 1)) { cfgpp_set_error("ip_load: %s: %d axes, expected %d", key, ndim, sp.cdim >= 0 ? 2 : 1); return -2; }
        dim[0] = sh[0]; dim[1] = nd > 1 ? sh[1] : 0;
        const int kinds[2] = {sp.rdim, sp.cdim};
        for (int ax = 0; ax < nd; ++ax) {
            static const char* const NAMES[] = {"D", "E", "inner", "inner", "ff_inner", "cross_attention_dim"};
            long got = dim[ax]; const int kd = kinds[ax];
            if (kd == RK_CROSS) {
                if (got != cross) { cfgpp_set_error("ip_load: %s: shape [%ld, %ld], axis %d must be the UNet's cross_attention_dim = %ld", key, dim[0], dim[1], ax, cross); return -2; }
                continue;
            }
            if (kd == RK_2INNER) {
                if (got % 2 != 0 || (g.inner && got != 2L * g.inner)) {
                    cfgpp_set_error("ip_load: %s: %ld rows, to_kv has 2 * inner = %d rows (K rows, then V rows)", key, got, 2 * g.inner); return -2;
                }
                got /= 2;
            }
            int& known = kd == RK_D ? g.D : kd == RK_E ? g.E : kd == RK_FF ? g.ff : g.inner;
            if (got < 64 || got % 64 != 0) {
                cfgpp_set_error("ip_load: %s: shape [%ld, %ld]: %s = %ld must be a positive multiple of 64", key, dim[0], dim[1], NAMES[kd], got); return -2;
            }
            if (known && known != got) {
                cfgpp_set_error("ip_load: %s: shape [%ld, %ld]: %s = %ld, the tensors loaded before have %s = %d (every layer has layer 0's shapes)", key, dim[0],
                                dim[1], NAMES[kd], got, NAMES[kd], known);
                return -2;
            }
            known = (int)got;
        }
        void** slot = res_layer < 0 ? &u->res.g[res_slot] : &u->res.l[res_layer][res_slot];
        if (sp.cdim >= 0) {
            std::vector<half_t> h; to_half(h);
            if (int e = put(slot, h.data(), h.size() * sizeof(half_t))) return e;
        } else {
            std::vector<float> f; to_float(f);
            if (int e = put(slot, f.data(), f.size() * sizeof(float))) return e;
        }
        u->res.E = g.E; u->res.D = g.D; u->res.nq = g.nq; u->res.inner = g.inner; u->res.ff = g.ff;
        u->ip_kind = cfgpp_unet::IP_RESAMPLER;
        changed();
        return 0;
    }
    if (k == "image_proj.proj.weight") {
        if (ndim != 2 || shape[0] % cross != 0 || shape[0] / cross < 1 || shape[0] / cross > cfgpp_unet::IP_MAX || shape[1] < 64 || shape[1] % 64 != 0) {
            cfgpp_set_error("ip_load: %s: shape [%ld, %ld], expected [n_img * %ld, embed_dim] with 1 <= n_img <= %d image tokens and embed_dim a "
                            "multiple of 64", key, ndim > 0 ? shape[0] : 0, ndim > 1 ? shape[1] : 0, cross, cfgpp_unet::IP_MAX);
            return -2;
        }
        std::vector<half_t> h; to_half(h);
        if (int e = put((void**)&u->ip_wproj, h.data(), h.size() * sizeof(half_t))) return e;
        u->ip_proj_rows = shape[0]; u->ip_embed = (int)shape[1];
        u->ip_kind = cfgpp_unet::IP_LINEAR; changed();
        return 0;
    }
    if (k == "image_proj.proj.bias") {
        if (ndim != 1 || shape[0] % cross != 0 || shape[0] / cross < 1 || shape[0] / cross > cfgpp_unet::IP_MAX) {
            cfgpp_set_error("ip_load: %s: %ld elements, expected n_img * %ld with 1 <= n_img <= %d", key, n, cross, cfgpp_unet::IP_MAX); return -2;
        }
        std::vector<float> f; to_float(f);
        if (int e = put((void**)&u->ip_bproj, f.data(), f.size() * sizeof(float))) return e;
        u->ip_bias_rows = shape[0];
        u->ip_kind = cfgpp_unet::IP_LINEAR; changed();
        return 0;
    }
    if (k == "image_proj.norm.weight" || k == "image_proj.norm.bias") {
        if (ndim != 1 || shape[0] != cross) { cfgpp_set_error("ip_load: %s: %ld elements, expected cross_attention_dim = %ld", key, n, cross); return -2; }
        std::vector<float> f; to_float(f);
        if (int e = put((void**)(k == "image_proj.norm.weight" ? &u->ip_ng : &u->ip_nb), f.data(), f.size() * sizeof(float))) return e;
        u->ip_kind = cfgpp_unet::IP_LINEAR; changed();
        return 0;
    }
    for (int part = 0; part < 2; ++part) {
        const std::string suf = part == 0 ? ".to_k_ip.weight" : ".to_v_ip.weight";
        if (k.size() <= suf.size() || k.compare(k.size() - suf.size(), suf.size(), suf) != 0) continue;
        const std::string blk = k.substr(0, k.size() - suf.size());
        for (auto& b : u->ip_blocks) {
            if (b.name != blk) continue;
            if (ndim != 2 || shape[0] != b.C || shape[1] != cross) {
                cfgpp_set_error("ip_load: %s: shape [%ld, %ld], expected [%d, %ld]", key, ndim > 0 ? shape[0] : 0, ndim > 1 ? shape[1] : 0, b.C, cross);
                return -2;
            }
            if (!b.wkv) {
                b.wkv = (half_t*)u->ip_malloc((size_t)2 * b.C * cross * sizeof(half_t));
                if (!b.wkv) return ip_fail(key, "out of device memory");
                CFGPP_HIP_CHECK(hipMemset(b.wkv, 0, (size_t)2 * b.C * cross * sizeof(half_t)));
            }
            std::vector<half_t> h; to_half(h);
            CFGPP_HIP_CHECK(hipDeviceSynchronize());
            CFGPP_HIP_CHECK(hipMemcpy(b.wkv + (size_t)part * b.C * cross, h.data(), h.size() * sizeof(half_t), hipMemcpyHostToDevice));
            (part == 0 ? b.has_k : b.has_v) = true;
            changed();
            return 0;
        }
    }
    cfgpp_set_error("ip_load: unknown key %s (image_proj.proj.{weight,bias}, image_proj.norm.{weight,bias}, <transformer block>.attn2.to_k_ip.weight / "
                    ".to_v_ip.weight; Resampler adapters: the image_proj.* keys of include/cfgpp_ip_plus.h)", key);
    return -3;
}

// the per-block half of an image context: u->ip_tok [rows][n_img][cross] -> every cross-attention's image K / V^T slots
static int ip_project_blocks(cfgpp_unet* u, int rows, int n_img, hipStream_t s) {
    const int cross = u->cfg.cross_attention_dim;
    for (const auto& b : u->ip_blocks) {
        // slots [96, 128) cleared first: a smaller n_img after a larger one leaves no stale keys
        if (int e = cfgpp_op_attention_clear_slots(b.ck, b.cvt, u->max_rows * b.nheads, b.d, u->ip_ck_pad, cfgpp_unet::IP_SLOT, cfgpp_unet::IP_MAX, s)) return e;
        IGemmArgs a = base_args(u);     // the form of the text K / V^T launch of ctx_plan, the image tokens as the batch's rows
        a.a0 = u->ip_tok; a.C0 = cross; a.amode = 0; a.w = b.wkv; a.N = 2 * b.C; a.K = cross; a.epi = EPI_HEADS;
        a.hq = nullptr; a.hk = b.ck + (size_t)cfgpp_unet::IP_SLOT * b.dp; a.hvt = b.cvt + cfgpp_unet::IP_SLOT;
        a.part0 = 1; a.part_width = b.C; a.head_dim = b.d; a.head_dim_pad = b.dp; a.heads = b.nheads;
        a.tok_pad = u->ip_ck_pad; a.q_tok_pad = u->ip_ck_pad; a.rows_per_batch = n_img; a.M = rows * n_img;
        if (int e = igemm_launch(a, s)) return e;
    }
    return 0;
}

// Replaces, per job instead of per step and per block: `image_embeds = self.encoder_hid_proj(image_embeds)` (ImageProjection.forward)
// of UNet2DConditionModel.process_encoder_hidden_states and `ip_key = self.to_k_ip[i](ip_hidden_states)` / `ip_value = ...` of
// IPAdapterAttnProcessor2_0.__call__; the per-step part (second SDPA + `hidden_states + scale * ip_hidden_states`) is the attention
// op of the plan.  No reference counterpart.
int cfgpp_unet_image_context(cfgpp_unet* u, const void* image_embeds, int rows, int embed_dim, float scale, void* stream) {
    CFGPP_REQUIRE(u && u->finalized, "image_context: engine not finalized");
    CFGPP_REQUIRE(!u->control, "image_context: a ControlNet takes no image tokens");
    if (!image_embeds || scale == 0.f) {            // deactivate: the next forward is the text-only plan, launch for launch
        if (u->ip_active) u->ip_set_active(false, 0, 0.f);
        return 0;
    }
    CFGPP_REQUIRE(u->ip_kind != cfgpp_unet::IP_RESAMPLER, "image_context: the loaded adapter is a Resampler (\"plus\") adapter: call "
                  "cfgpp_unet_image_context_seq with the image tower's hidden states [rows][seq][embed_dim] (include/cfgpp_ip_plus.h)");
    {
        std::string miss; int nm = 0;
        auto need = [&](bool have, const std::string& name) { if (!have) { if (nm < 8) miss += name + " "; ++nm; } };
        need(u->ip_wproj, "image_proj.proj.weight"); need(u->ip_bproj, "image_proj.proj.bias");
        need(u->ip_ng, "image_proj.norm.weight"); need(u->ip_nb, "image_proj.norm.bias");
        for (const auto& b : u->ip_blocks) { need(b.has_k, b.name + ".to_k_ip.weight"); need(b.has_v, b.name + ".to_v_ip.weight"); }
        if (nm) { cfgpp_set_error("image_context: missing %d adapter tensors (cfgpp_unet_ip_load): %s%s", nm, miss.c_str(), nm > 8 ? "..." : ""); return -2; }
    }
    CFGPP_REQUIRE(u->ip_bias_rows == u->ip_proj_rows, "image_context: image_proj.proj.bias has %ld elements, image_proj.proj.weight %ld rows",
                  u->ip_bias_rows, u->ip_proj_rows);
    CFGPP_REQUIRE(embed_dim == u->ip_embed, "image_context: embed_dim=%d, the adapter's image_proj.proj takes %d", embed_dim, u->ip_embed);
    CFGPP_REQUIRE(u->ctx_set && rows == u->ctx_rows, "image_context: rows=%d must equal the rows of the current text context (%d): call "
                  "cfgpp_unet_set_context first", rows, u->ctx_set ? u->ctx_rows : 0);
    const int cross = u->cfg.cross_attention_dim, n_img = (int)(u->ip_proj_rows / cross);
    hipStream_t s = (hipStream_t)stream;
    CFGPP_HIP_CHECK(hipSetDevice(u->device));
    if (!(u->ip_src == image_embeds && u->ip_rows == rows)) {       // (a new scale alone keeps the projected K / V^T)
        const long need_el = (long)u->max_rows * n_img * cross;
        if (u->ip_tok_cap < need_el) {
            CFGPP_HIP_CHECK(hipDeviceSynchronize());
            if (u->ip_proj_out) u->ip_free(u->ip_proj_out);
            if (u->ip_tok) u->ip_free(u->ip_tok);
            u->ip_proj_out = (half_t*)u->ip_malloc((size_t)need_el * sizeof(half_t));
            u->ip_tok = (half_t*)u->ip_malloc((size_t)need_el * sizeof(half_t));
            u->ip_tok_cap = (u->ip_proj_out && u->ip_tok) ? need_el : 0;
            CFGPP_REQUIRE(u->ip_tok_cap, "image_context: out of device memory");
        }
        u->ip_src = nullptr;
        {   // tokens = LayerNorm(reshape(proj(embeds), [rows, n_img, cross_dim]))
            IGemmArgs a = base_args(u);
            a.a0 = (const half_t*)image_embeds; a.C0 = embed_dim; a.amode = 0; a.w = u->ip_wproj; a.N = n_img * cross; a.K = embed_dim;
            a.bias = u->ip_bproj; a.rmode = 0; a.rld = a.N; a.out = u->ip_proj_out; a.omode = 0; a.old = a.N; a.epi = EPI_STORE;
            a.rows_per_batch = rows; a.M = rows;
            if (int e = igemm_launch(a, s)) return e;
            if (int e = cfgpp_op_layernorm(u->ip_proj_out, u->ip_tok, u->ip_ng, u->ip_nb, (long)rows * n_img, cross, 1e-5f, s)) return e;
        }
        if (int e = ip_project_blocks(u, rows, n_img, s)) return e;
        u->ip_src = image_embeds; u->ip_rows = rows;
    }
    u->ip_set_active(true, n_img, scale);
    return 0;
}

// The Resampler form of the call above (include/cfgpp_ip_plus.h): replaces, per job, `image_embeds = self.encoder_hid_proj(image_embeds)`
// with encoder_hid_proj an IP-Adapter Resampler (PerceiverAttention + FeedForward layers over learned latents).  Dataflow, all fp16
// between launches (x, xn, kv_x sized by seq; the rest by n_q):
//   x = proj_in(hidden) + b                                      GEMM, bias in the epilogue
//   lat = fp16(latents) for every row                            broadcast_rows
//   per layer:  xn = LN(x; norm1)   ln = LN(lat; norm2)          cfgpp_op_layernorm
//               q = to_q(ln)   kv_x = to_kv(xn)   kv_l = to_kv(ln)      three GEMMs, token-major outputs
//               att = perceiver attention(q, kv_x, kv_l)          resampler.hip, reads those outputs as they are
//               lat = to_out(att) + lat                           GEMM, residual in the epilogue (in place)
//               ln = LN(lat; ff norm)   ff = W1(ln)   ff = gelu_erf(ff)   lat = W2(ff) + lat
//   tokens = LN(proj_out(lat) + b; norm_out)  -> u->ip_tok
int cfgpp_unet_image_context_seq(cfgpp_unet* u, const void* hidden, int rows, int seq, int embed_dim, float scale, void* stream) {
    CFGPP_REQUIRE(u && u->finalized, "image_context_seq: engine not finalized");
    CFGPP_REQUIRE(!u->control, "image_context_seq: a ControlNet takes no image tokens");
    if (!hidden || scale == 0.f) {                  // deactivate: the next forward is the text-only plan, launch for launch
        if (u->ip_active) u->ip_set_active(false, 0, 0.f);
        return 0;
    }
    CFGPP_REQUIRE(u->ip_kind != cfgpp_unet::IP_LINEAR, "image_context_seq: the loaded adapter has a Linear + LayerNorm image projection: call "
                  "cfgpp_unet_image_context with the pooled embeds [rows][embed_dim]");
    cfgpp_unet::Resampler& R = u->res;
    int depth = 0;
    for (int i = 0; i < cfgpp_unet::RES_MAX_DEPTH; ++i)
        for (int j = 0; j < cfgpp_unet::RL_COUNT; ++j) if (R.l[i][j]) depth = i + 1;
    {
        std::string miss; int nm = 0;
        auto need = [&](bool have, const std::string& name) { if (!have) { if (nm < 8) miss += name + " "; ++nm; } };
        for (int j = 0; j < cfgpp_unet::RG_COUNT; ++j) need(R.g[j], std::string("image_proj.") + RES_GLOBAL[j].name);
        for (int i = 0; i < (depth ? depth : 1); ++i)
            for (int j = 0; j < cfgpp_unet::RL_COUNT; ++j) need(R.l[i][j], "image_proj.layers." + std::to_string(i) + "." + RES_LAYER[j].name);
        for (const auto& b : u->ip_blocks) { need(b.has_k, b.name + ".to_k_ip.weight"); need(b.has_v, b.name + ".to_v_ip.weight"); }
        if (nm) { cfgpp_set_error("image_context_seq: missing %d adapter tensors (cfgpp_unet_ip_load): %s%s", nm, miss.c_str(), nm > 8 ? "..." : ""); return -2; }
    }
    CFGPP_REQUIRE(embed_dim == R.E, "image_context_seq: embed_dim=%d, the adapter's image_proj.proj_in takes %d", embed_dim, R.E);
    CFGPP_REQUIRE(seq >= 1 && seq <= 1024, "image_context_seq: seq=%d (1 .. 1024 hidden-state tokens per row)", seq);
    CFGPP_REQUIRE(u->ctx_set && rows == u->ctx_rows, "image_context_seq: rows=%d must equal the rows of the current text context (%d): call "
                  "cfgpp_unet_set_context first", rows, u->ctx_set ? u->ctx_rows : 0);
    const int cross = u->cfg.cross_attention_dim, nq = R.nq, D = R.D, inner = R.inner, ff = R.ff, heads = R.inner / 64;
    hipStream_t s = (hipStream_t)stream;
    CFGPP_HIP_CHECK(hipSetDevice(u->device));
    if (!(u->ip_src == hidden && u->ip_rows == rows && u->ip_seq == seq)) {     // (a new scale alone keeps the projected K / V^T)
        const long Ml_cap = (long)u->max_rows * nq;
        if (!R.ls || !u->ip_tok) {
            CFGPP_HIP_CHECK(hipDeviceSynchronize());
            if (!R.ls) R.ls = (half_t*)u->ip_malloc((size_t)Ml_cap * (2 * D + 4 * inner + ff + cross) * sizeof(half_t));
            if (!u->ip_tok) u->ip_tok = (half_t*)u->ip_malloc((size_t)Ml_cap * cross * sizeof(half_t));
            u->ip_tok_cap = (R.ls && u->ip_tok) ? Ml_cap * cross : 0;
            CFGPP_REQUIRE(u->ip_tok_cap, "image_context_seq: out of device memory");
        }
        if (R.S_cap < seq) {                        // the seq-sized activations grow, never shrink
            CFGPP_HIP_CHECK(hipDeviceSynchronize());
            if (R.xs) u->ip_free(R.xs);
            R.xs = (half_t*)u->ip_malloc((size_t)u->max_rows * seq * (2 * D + 2 * inner) * sizeof(half_t));
            R.S_cap = R.xs ? seq : 0;
            CFGPP_REQUIRE(R.xs, "image_context_seq: out of device memory");
        }
        u->ip_src = nullptr;
        const int Mx = rows * seq, Ml = rows * nq;
        half_t* x = R.xs; half_t* xn = x + (long)Mx * D; half_t* kvx = xn + (long)Mx * D;
        half_t* lat = R.ls; half_t* ln = lat + (long)Ml * D; half_t* q = ln + (long)Ml * D; half_t* kvl = q + (long)Ml * inner;
        half_t* att = kvl + (long)Ml * 2 * inner; half_t* ffb = att + (long)Ml * inner; half_t* po = ffb + (long)Ml * ff;
        auto gemm = [&](const half_t* A, int tokens, int K, const void* w, int N, const void* bias, const half_t* resid, half_t* out) {
            IGemmArgs a = base_args(u);
            a.a0 = A; a.C0 = K; a.amode = 0; a.w = (const half_t*)w; a.N = N; a.K = K; a.bias = (const float*)bias;
            a.resid = resid; a.rmode = 0; a.rld = N; a.out = out; a.omode = 0; a.old = N; a.epi = EPI_STORE;
            a.rows_per_batch = tokens; a.M = rows * tokens;
            return igemm_launch(a, s);
        };
        auto norm = [&](const half_t* in, half_t* out, const void* g, const void* b, long n, int C) {
            return cfgpp_op_layernorm(in, out, (const float*)g, (const float*)b, n, C, 1e-5f, s);
        };
        if (int e = gemm((const half_t*)hidden, seq, embed_dim, R.g[cfgpp_unet::RG_PIN_W], D, R.g[cfgpp_unet::RG_PIN_B], nullptr, x)) return e;
        if (int e = broadcast_rows_launch((const float*)R.g[cfgpp_unet::RG_LATENTS], lat, (long)nq * D, rows, s)) return e;
        for (int i = 0; i < depth; ++i) {
            void* const* L = R.l[i];
            if (int e = norm(x, xn, L[cfgpp_unet::RL_N1_W], L[cfgpp_unet::RL_N1_B], Mx, D)) return e;
            if (int e = norm(lat, ln, L[cfgpp_unet::RL_N2_W], L[cfgpp_unet::RL_N2_B], Ml, D)) return e;
            if (int e = gemm(ln, nq, D, L[cfgpp_unet::RL_Q], inner, nullptr, nullptr, q)) return e;
            if (int e = gemm(xn, seq, D, L[cfgpp_unet::RL_KV], 2 * inner, nullptr, nullptr, kvx)) return e;
            if (int e = gemm(ln, nq, D, L[cfgpp_unet::RL_KV], 2 * inner, nullptr, nullptr, kvl)) return e;
            if (int e = perceiver_attn_launch(q, kvx, kvl, att, rows, heads, nq, seq, s)) return e;
            if (int e = gemm(att, nq, inner, L[cfgpp_unet::RL_OUT], D, nullptr, lat, lat)) return e;
            if (int e = norm(lat, ln, L[cfgpp_unet::RL_FN_W], L[cfgpp_unet::RL_FN_B], Ml, D)) return e;
            if (int e = gemm(ln, nq, D, L[cfgpp_unet::RL_FF1], ff, nullptr, nullptr, ffb)) return e;
            if (int e = gelu_inplace_launch(ffb, (long)Ml * ff, s)) return e;
            if (int e = gemm(ffb, nq, ff, L[cfgpp_unet::RL_FF2], D, nullptr, lat, lat)) return e;
        }
        if (int e = gemm(lat, nq, D, R.g[cfgpp_unet::RG_POUT_W], cross, R.g[cfgpp_unet::RG_POUT_B], nullptr, po)) return e;
        if (int e = norm(po, u->ip_tok, R.g[cfgpp_unet::RG_NOUT_W], R.g[cfgpp_unet::RG_NOUT_B], Ml, cross)) return e;
        if (int e = ip_project_blocks(u, rows, nq, s)) return e;
        u->ip_src = hidden; u->ip_rows = rows; u->ip_seq = seq;
    }
    u->ip_set_active(true, nq, scale);
    return 0;
}

int cfgpp_unet_ip_tokens(cfgpp_unet* u, void* host_fp16_out, int rows) {
    CFGPP_REQUIRE(u && u->finalized && host_fp16_out, "ip_tokens: null engine / output");
    CFGPP_REQUIRE(u->ip_tok && u->ip_src, "ip_tokens: no image tokens computed since the adapter was loaded (cfgpp_unet_image_context / _seq)");
    CFGPP_REQUIRE(rows == u->ip_rows, "ip_tokens: rows=%d, the last image context had %d", rows, u->ip_rows);
    const long cross = u->cfg.cross_attention_dim;
    const long n_img = u->ip_kind == cfgpp_unet::IP_RESAMPLER ? u->res.nq : u->ip_proj_rows / cross;
    CFGPP_HIP_CHECK(hipSetDevice(u->device));
    CFGPP_HIP_CHECK(hipDeviceSynchronize());
    CFGPP_HIP_CHECK(hipMemcpy(host_fp16_out, u->ip_tok, (size_t)rows * n_img * cross * sizeof(half_t), hipMemcpyDeviceToHost));
    return 0;
}

int cfgpp_unet_attach_control(cfgpp_unet* u, cfgpp_unet* cn, float scale) {
    CFGPP_REQUIRE(u && u->finalized, "attach_control: UNet not finalized");
    CFGPP_REQUIRE(!u->control, "attach_control: the target is itself a ControlNet");
    if (!cn) { u->ctrl = nullptr; u->ctrl_scale = 0.f; return 0; }
    CFGPP_REQUIRE(cn->finalized && cn->control, "attach_control: not a finalized ControlNet (cfgpp_unet_create with out_channels = 0, then finalize)");
    const cfgpp_unet_config &a = u->cfg, &b = cn->cfg;
    CFGPP_REQUIRE(a.num_levels == b.num_levels && a.layers_per_block == b.layers_per_block, "attach_control: levels %d x %d vs the UNet's %d x %d",
                  b.num_levels, b.layers_per_block, a.num_levels, a.layers_per_block);
    for (int i = 0; i < a.num_levels; ++i)
        CFGPP_REQUIRE(a.block_out_channels[i] == b.block_out_channels[i], "attach_control: channels of level %d: %d vs the UNet's %d", i,
                      b.block_out_channels[i], a.block_out_channels[i]);
    CFGPP_REQUIRE(a.sample_h == b.sample_h && a.sample_w == b.sample_w, "attach_control: latent %d x %d vs the UNet's %d x %d", b.sample_h,
                  b.sample_w, a.sample_h, a.sample_w);
    CFGPP_REQUIRE(a.max_rows == b.max_rows, "attach_control: max_rows %d vs the UNet's %d", b.max_rows, a.max_rows);
    CFGPP_REQUIRE(b.in_channels == a.out_channels, "attach_control: the ControlNet takes %d latent channels, the UNet %d", b.in_channels,
                  a.out_channels);
    CFGPP_REQUIRE(cn->ctrl_res.size() == u->ctrl_dst.size(), "attach_control: %d residuals for %d skip connections + mid block",
                  (int)cn->ctrl_res.size(), (int)u->ctrl_dst.size());
    std::vector<CnAddEntry> tab(u->ctrl_dst.size());
    for (size_t i = 0; i < tab.size(); ++i) {
        const Tensor &d = u->ctrl_dst[i], &r = cn->ctrl_res[i];
        CFGPP_REQUIRE(d.H == r.H && d.W == r.W && d.C == r.C, "attach_control: residual %d is %d x %d x %d, the UNet tensor %d x %d x %d", (int)i,
                      r.H, r.W, r.C, d.H, d.W, d.C);
        tab[i] = CnAddEntry{d.p, r.p, d.H, d.W, d.C, 0};
    }
    CFGPP_HIP_CHECK(hipSetDevice(u->device));
    CFGPP_HIP_CHECK(hipDeviceSynchronize());         // an earlier forward may still read the table
    CFGPP_HIP_CHECK(hipMemcpy(u->d_ctrl_tab, tab.data(), tab.size() * sizeof(CnAddEntry), hipMemcpyHostToDevice));
    u->ctrl = cn; u->ctrl_scale = scale;
    return 0;
}

int cfgpp_controlnet_residual(cfgpp_unet* cn, int i, float scale, float* out, int rows, int* hwc_out, void* stream) {
    CFGPP_REQUIRE(cn && cn->finalized && cn->control, "controlnet_residual: not a finalized ControlNet");
    const int n = (int)cn->ctrl_res.size();
    if (!out && !hwc_out) return n;
    CFGPP_REQUIRE(i >= 0 && i < n, "controlnet_residual: index %d (0 .. %d)", i, n - 1);
    const Tensor& r = cn->ctrl_res[i];
    if (hwc_out) { hwc_out[0] = r.H; hwc_out[1] = r.W; hwc_out[2] = r.C; }
    if (!out) return n;
    CFGPP_REQUIRE(rows > 0 && rows <= cn->cfg.max_rows, "controlnet_residual: rows=%d", rows);
    int e = cfgpp_op_residual_nchw(r.p, out, rows, r.H, r.W, r.C, scale, stream);
    return e ? e : n;
}

int cfgpp_unet_forward(cfgpp_unet* u, const void* z, int z_is_half, int z_rows, float t, void* eps_out, int rows,
                       void* stream) {
    CFGPP_REQUIRE(u && u->finalized, "forward: context not finalized");
    CFGPP_REQUIRE(u->ctx_set, "forward: set_context has not been called");
    CFGPP_REQUIRE(!u->time_cond || u->time_cond_set, "forward: a guidance-embedded UNet (time_cond_proj_dim=%d) needs "
                  "cfgpp_unet_guidance_embedding first", u->time_cond);
    CFGPP_REQUIRE(z && eps_out && z_rows > 0 && rows > 0 && rows <= u->cfg.max_rows, "forward: bad args (rows=%d max=%d)", rows, u->cfg.max_rows);
    CFGPP_REQUIRE(rows == u->ctx_rows, "forward: rows=%d but context was set for %d rows", rows, u->ctx_rows);
    CFGPP_REQUIRE(u->control || u->cfg.in_channels == u->cfg.out_channels || (u->cond_rows > 0 && (u->cond_rows == 1 || u->cond_rows == z_rows)),
                  "forward: inpaint UNet (%d input channels) needs cfgpp_unet_image_condition with 1 or z_rows=%d rows first (has %d)",
                  u->cfg.in_channels, z_rows, u->cond_rows);
    CFGPP_REQUIRE(!u->control || u->img_rows > 0, "forward: ControlNet without a control image (call cfgpp_unet_image_condition first)");
    CFGPP_REQUIRE(!u->ip_active || u->ip_rows == rows, "forward: the image context (IP-Adapter) was set for %d rows, the forward runs %d: call "
                  "cfgpp_unet_image_context after cfgpp_unet_set_context", u->ip_rows, rows);
    if (int e = regions_ready(u, rows, "forward")) return e;
    if (u->ctrl && u->ctrl_scale != 0.f) {         // the attached ControlNet's forward first: its residuals feed this plan
        cfgpp_unet* cn = u->ctrl;
        CFGPP_REQUIRE(cn->img_rows > 0, "forward: a ControlNet is attached but has no control image (cfgpp_unet_image_condition)");
        CFGPP_REQUIRE(cn->ctx_set && cn->ctx_rows == rows, "forward: the attached ControlNet's context is set for %d rows, the forward runs %d",
                      cn->ctx_set ? cn->ctx_rows : 0, rows);
        int e = cfgpp_unet_forward(cn, z, z_is_half, z_rows, t, eps_out, rows, stream);
        if (e) return e;
    }
    u->in_z = z; u->in_z_half = z_is_half; u->in_z_rows = z_rows; u->in_t = t; u->in_t_dev = nullptr; u->out_eps = eps_out;
    const bool shared = u->enter_call(rows, z_rows);
    if ((u->tuned_rows != rows || u->tuned_shared != shared) && igemm_autotune_enabled()) {      // first forward at this batch and mode: in-situ tile tuning
        int e = u->tune_plan((hipStream_t)stream, rows, shared); if (e) return e;
        ++u->tuned_serial;
    }
    for (size_t i = 0; i < u->plan.size(); ++i) { int e = u->plan[i]((hipStream_t)stream, u->rows_for(i, rows, shared)); if (e) return e; }
    return 0;
}

// Whole-loop graph replay: the reference's DDIM loops with callback_fn None
// (latent_diffusion.py:653-674, 272-294, 160-182; latent_sdxl.py:730-752, 838-858) as ONE captured step - UNet forward at `rows` +
// the fused generalised DDIM update - replayed n_steps times.  The per-step scalars {t, c1, c2, c3, c4} (host_steps[n_steps][5],
// the same fp32 values cfgpp_unet_forward / cfgpp_step_ddim take as arguments) go into a device table; the graph's first node
// copies the current row and advances a device counter, so one graph serves every step and every later call with the same
// buffers.  z / z0t [z_rows,4,H,W] fp32 or fp16 (updated in place / written per step), eps [rows,4,H,W] fp16 scratch the UNet
// writes, eps_uc / eps_c point into it.  Capture happens on an engine-owned stream (the caller's may be the legacy default
// stream, which cannot capture) after one eager forward (tile tuning, lazy kernel attributes); replays are enqueued on `stream`.
// Results are bit-identical to the eager loop.  Returns 0, < 0 on error (a failed capture leaves no graph behind).
int cfgpp_sample_graph_ddim(cfgpp_unet* u, void* z, void* z0t, int z_is_half, int z_rows, void* eps, const void* eps_uc,
                            const void* eps_c, int rows, const float* host_steps, int n_steps, float lam, int tweedie_uc,
                            int renoise_uc, void* stream) {
    CFGPP_REQUIRE(u && u->finalized && u->ctx_set, "sample_graph: context not ready");
    CFGPP_REQUIRE(z && z0t && eps && eps_uc && eps_c && host_steps && n_steps > 0 && z_rows > 0, "sample_graph: bad args");
    CFGPP_REQUIRE(!u->time_cond || u->time_cond_set, "sample_graph: a guidance-embedded UNet (time_cond_proj_dim=%d) needs "
                  "cfgpp_unet_guidance_embedding first", u->time_cond);
    CFGPP_REQUIRE(rows == u->ctx_rows && rows <= u->cfg.max_rows, "sample_graph: rows=%d but context was set for %d rows", rows, u->ctx_rows);
    CFGPP_REQUIRE(!u->ctrl && !u->control, "sample_graph: a ControlNet is attached (a controlled step is not captured): detach it "
                                            "(cfgpp_unet_attach_control(u, NULL, 0)) or run the eager loop");
    CFGPP_REQUIRE(!u->regions, "sample_graph: regional prompts are on (cfgpp_unet_set_regions, n_regions=%d): a region-masked step is not captured, "
                                "run the eager loop", u->regions);
    CFGPP_REQUIRE(!u->soft_regions, "sample_graph: region weights are on (cfgpp_unet_set_region_weights, n_regions=%d): a region-weighted step is not "
                                     "captured, run the eager loop", u->soft_regions);
    hipStream_t s = (hipStream_t)stream;
    CFGPP_REQUIRE(u->cfg.in_channels == u->cfg.out_channels || (u->cond_rows > 0 && (u->cond_rows == 1 || u->cond_rows == z_rows)),
                  "sample_graph: inpaint UNet (%d input channels) needs cfgpp_unet_image_condition with 1 or z_rows=%d rows first (has %d)",
                  u->cfg.in_channels, z_rows, u->cond_rows);
    const long n = (long)z_rows * u->cfg.out_channels * u->cfg.sample_h * u->cfg.sample_w;
    if (!u->d_step_cur) {
        u->d_step_cur = (float*)u->dmalloc(8 * sizeof(float));
        u->d_step_idx = (int*)u->dmalloc(sizeof(int));
        CFGPP_REQUIRE(u->d_step_cur && u->d_step_idx, "sample_graph: out of device memory");
        CFGPP_HIP_CHECK(hipStreamCreateWithFlags(&u->cap_stream, hipStreamNonBlocking));
    }
    if (n_steps > u->step_tab_cap) {
        u->drop_graphs();                                         // the graphs hold the old table's address
        const int cap = n_steps < 64 ? 64 : n_steps;
        u->d_step_tab = (float*)u->dmalloc((size_t)cap * 8 * sizeof(float));   // (the old table is freed with the engine)
        CFGPP_REQUIRE(u->d_step_tab, "sample_graph: out of device memory");
        u->step_tab_cap = cap;
    }
    u->enter_call(rows, z_rows);           // a graph captured in the other mode (switch flipped since) must not hit: the serial moves
    CFGPP_REQUIRE(!u->ip_active || u->ip_rows == rows, "sample_graph: the image context (IP-Adapter) was set for %d rows, the loop runs %d", u->ip_rows, rows);
    cfgpp_unet::GraphKey want{z, z0t, eps, eps_uc, eps_c, z_is_half, z_rows, rows, tweedie_uc, renoise_uc, lam, n, 0, u->cond_rows};
    want.ip_active = u->ip_active ? 1 : 0; want.ip_n_img = u->ip_n_img; std::memcpy(&want.ip_scale_bits, &u->ip_scale, sizeof(float));
    want.ctx_tokens = u->ctx_tokens;
    want.freeu_on = u->freeu_on ? 1 : 0;
    if (u->freeu_on) {
        const float f[4] = {u->freeu_s[0], u->freeu_s[1], u->freeu_b[0], u->freeu_b[1]};
        std::memcpy(want.freeu_bits, f, sizeof(f));
    }
    auto same = [&](const cfgpp_unet::GraphKey& k) {
        return k.z == want.z && k.z0t == want.z0t && k.eps == want.eps && k.euc == want.euc && k.ec == want.ec && k.z_half == want.z_half &&
               k.z_rows == want.z_rows && k.rows == want.rows && k.tw == want.tw && k.rn == want.rn && k.lam == want.lam && k.n == want.n &&
               k.tuned_serial == u->tuned_serial && k.cond_rows == want.cond_rows && k.ip_active == want.ip_active &&
               k.ip_n_img == want.ip_n_img && k.ip_scale_bits == want.ip_scale_bits && k.ctx_tokens == want.ctx_tokens &&
               k.freeu_on == want.freeu_on && std::memcmp(k.freeu_bits, want.freeu_bits, sizeof(want.freeu_bits)) == 0;
    };
    int hit = -1;
    for (size_t i = 0; i < u->graphs.size(); ++i) if (same(u->graphs[i].key)) hit = (int)i;
    if (hit < 0) {
        // eager first: tile tuning (bumps tuned_serial), kernel attributes and every other lazy host-side initialisation happen
        // outside the capture.  The forward only reads z, so the loop below starts from the same state.
        int e = cfgpp_unet_forward(u, z, z_is_half, z_rows, host_steps[0], eps, rows, stream);
        if (e) return e;
        CFGPP_HIP_CHECK(hipStreamSynchronize(s));
        for (size_t i = 0; i < u->graphs.size();)                 // graphs of other pins can never hit again
            if (u->graphs[i].key.tuned_serial != u->tuned_serial) { cfgpp_unet::destroy(u->graphs[i]); u->graphs.erase(u->graphs.begin() + i); } else ++i;
        cfgpp_unet::Graph g{want, nullptr, nullptr};
        g.key.tuned_serial = u->tuned_serial;
        u->in_t_dev = u->d_step_cur;
        hipError_t he = hipStreamBeginCapture(u->cap_stream, hipStreamCaptureModeRelaxed);
        int rc = 0;
        if (he == hipSuccess) {
            rc = step_advance_launch(u->d_step_tab, u->d_step_idx, u->d_step_cur, u->cap_stream);
            const bool shared = u->shares(rows, z_rows);      // the mode of the eager forward above
            for (size_t i = 0; i < u->plan.size() && rc == 0; ++i) rc = u->plan[i](u->cap_stream, u->rows_for(i, rows, shared));
            if (rc == 0) rc = step_ddim_dev_launch(z, z0t, eps_uc, eps_c, 1, z_is_half, lam, u->d_step_cur + 1, tweedie_uc, renoise_uc, n, u->cap_stream);
            he = hipStreamEndCapture(u->cap_stream, &g.graph);
        }
        u->in_t_dev = nullptr;
        if (he != hipSuccess || rc != 0 || !g.graph) {
            cfgpp_unet::destroy(g);
            if (rc == 0) cfgpp_set_error("sample_graph: stream capture failed: %s", hipGetErrorString(he));
            return rc ? rc : -1;
        }
        he = hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0);
        if (he != hipSuccess) { cfgpp_unet::destroy(g); cfgpp_set_error("sample_graph: hipGraphInstantiate: %s", hipGetErrorString(he)); return -1; }
        if (u->graphs.size() >= 4) { cfgpp_unet::destroy(u->graphs.front()); u->graphs.erase(u->graphs.begin()); }
        u->graphs.push_back(g);
        hit = (int)u->graphs.size() - 1;
    }
    if (hit != (int)u->graphs.size() - 1) std::swap(u->graphs[hit], u->graphs.back());
    hipGraphExec_t exec = u->graphs.back().exec;
    // this call's table (pageable host memory: the copy is staged, the buffer is free when the call returns) and counter
    std::vector<float> tab((size_t)n_steps * 8, 0.f);
    for (int i = 0; i < n_steps; ++i) for (int k = 0; k < 5; ++k) tab[(size_t)i * 8 + k] = host_steps[(size_t)i * 5 + k];
    CFGPP_HIP_CHECK(hipMemcpyAsync(u->d_step_tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice, s));
    CFGPP_HIP_CHECK(hipStreamSynchronize(s));        // `tab` leaves scope; once per sampling loop
    CFGPP_HIP_CHECK(hipMemsetAsync(u->d_step_idx, 0, sizeof(int), s));
    for (int i = 0; i < n_steps; ++i) CFGPP_HIP_CHECK(hipGraphLaunch(exec, s));
    return 0;
}

// One forward with a HIP event between every launch of the plan, on `stream` (the stream the
// kernels run on).  out_ms[k] / out_flops[k] / out_launches[k], k = 0 igemm (conv/linear),
// 1 attention, 2 norm (GroupNorm/LayerNorm), 3 small ops; flops are ALGORITHMIC (2*MAC).
int cfgpp_unet_profile(cfgpp_unet* u, const void* z, int z_is_half, int z_rows, float t, void* eps_out, int rows,
                       void* stream, double* out_ms, double* out_flops, int* out_launches, char* detail, long detail_cap) {
    CFGPP_REQUIRE(u && u->finalized && u->ctx_set, "profile: context not ready");
    CFGPP_REQUIRE(z && eps_out && out_ms && out_flops && out_launches && rows == u->ctx_rows, "profile: bad args");
    CFGPP_REQUIRE(!u->time_cond || u->time_cond_set, "profile: a guidance-embedded UNet (time_cond_proj_dim=%d) needs "
                  "cfgpp_unet_guidance_embedding first", u->time_cond);
    CFGPP_REQUIRE(!u->ip_active || u->ip_rows == rows, "profile: the image context (IP-Adapter) was set for %d rows", u->ip_rows);
    if (int e = regions_ready(u, rows, "profile")) return e;
    u->in_z = z; u->in_z_half = z_is_half; u->in_z_rows = z_rows; u->in_t = t; u->out_eps = eps_out;
    hipStream_t s = (hipStream_t)stream;
    const size_t n = u->plan.size();
    // the rows every op really runs at: times, FLOPs and descriptions below are those of the work that was done.  (The tiles are
    // whatever the last forward pinned: profile after a forward of the same mode.)
    const bool shared = u->enter_call(rows, z_rows);
    std::vector<int> op_rows(n);
    for (size_t i = 0; i < n; ++i) op_rows[i] = u->rows_for(i, rows, shared);
    std::vector<hipEvent_t> ev(n + 1);
    for (auto& e : ev) CFGPP_HIP_CHECK(hipEventCreate(&e));
    CFGPP_HIP_CHECK(hipEventRecord(ev[0], s));
    int rc = 0;
    for (size_t i = 0; i < n && rc == 0; ++i) { rc = u->plan[i](s, op_rows[i]); if (rc == 0 && hipEventRecord(ev[i + 1], s) != hipSuccess) rc = -1; }
    if (rc == 0 && hipStreamSynchronize(s) != hipSuccess) rc = -1;
    for (int k = 0; k < 4; ++k) { out_ms[k] = 0; out_flops[k] = 0; out_launches[k] = 0; }
    if (rc == 0) {
        for (size_t i = 0; i < n; ++i) {
            if (op_rows[i] == 0) continue;               // not part of this call (the fan-out of a call that does not share)
            float ms = 0.f; hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
            const int k = u->plan_kind[i];
            out_ms[k] += ms; out_flops[k] += 2.0 * u->plan_macs[i] * op_rows[i]; out_launches[k] += 1;
        }
        if (detail && detail_cap > 0) {      // one line per launch: index, family, description, us, GFLOP
            std::string txt;
            for (size_t i = 0; i < n; ++i) {
                if (op_rows[i] == 0) continue;
                float ms = 0.f; hipEventElapsedTime(&ms, ev[i], ev[i + 1]);
                char line[256];
                const std::string desc = u->plan_desc[i] + (op_rows[i] != rows ? " rows=" + std::to_string(op_rows[i]) : std::string());
                snprintf(line, sizeof(line), "%zu\t%d\t%s\t%.1f\t%.3f\n", i, u->plan_kind[i], desc.c_str(), ms * 1e3,
                         2.0 * u->plan_macs[i] * op_rows[i] * 1e-9);
                txt += line;
            }
            const long ncopy = std::min<long>((long)txt.size(), detail_cap - 1);
            std::memcpy(detail, txt.data(), ncopy); detail[ncopy] = 0;
        }
    }
    for (auto& e : ev) hipEventDestroy(e);
    return rc;
}

// Export (set = 0) / import (set = 1) the tile configs the in-situ tuning pinned for batch `rows`: one int per
// igemm launch of the plan, in plan order.  Lets a profiled run (rocprofv3 --pmc) replay exactly the tiles of the
// un-profiled run without timing passes of its own.  Returns the number of hint slots, or < 0 on error.
int cfgpp_unet_tuning(cfgpp_unet* u, int rows, int* hints, int cap, int set) {
    CFGPP_REQUIRE(u && u->finalized && hints && rows > 0, "unet_tuning: bad args");
    const int n = (int)u->cfg_hints.size();
    CFGPP_REQUIRE(cap >= n, "unet_tuning: buffer of %d for %d launches", cap, n);
    if (set) {
        // an import may arrive before any forward, when the mode of the calls to come is not known: both modes of this batch get
        // the list (pins only decide speed, and a launch rejects a tile it cannot run)
        for (int sh = 0; sh < 2; ++sh) u->tuned_by_rows[std::make_pair(rows, sh != 0)] = std::vector<int>(hints, hints + n);
        if (u->tuned_rows == rows) u->tuned_rows = 0;      // re-install on the next forward
        ++u->tuned_serial;
        return n;
    }
    auto it = u->tuned_by_rows.find(std::make_pair(rows, u->ran_shared == 1));       // the mode the engine last ran in
    if (it == u->tuned_by_rows.end()) { cfgpp_set_error("unet_tuning: batch %d has not been tuned", rows); return -3; }
    std::copy(it->second.begin(), it->second.end(), hints);
    return n;
}

double cfgpp_unet_flops(cfgpp_unet* u, int rows) {
    if (!u || !u->finalized) return 0.0;
    // the prefix a CFG call shares is computed once for both halves: counted once when the most recent forward shared it
    const double once = u->ran_shared == 1 ? u->prefix_macs_per_row * (rows / 2) : 0.0;
    const double ip = u->ip_active ? u->ip_macs_per_key * u->ip_n_img : 0.0;      // the image keys, while an adapter is active
    // attn_macs_per_row counts 77 text keys per cross-attention; a regional row attends to its own 77 keys
    const double text = u->regions ? 0.0 : u->ip_macs_per_key * (u->ctx_tokens - 77);
    return 2.0 * ((u->macs_per_row + u->attn_macs_per_row + text + ip) * rows - once);
}

void cfgpp_unet_set_share_prefix(int on) { g_share_prefix = on ? 1 : 0; }
int cfgpp_unet_share_prefix_enabled(void) { return g_share_prefix; }
int cfgpp_unet_shared_prefix_ops(cfgpp_unet* u, int rows, int z_rows) {
    if (!u || !u->finalized) return 0;
    return u->shares(rows, z_rows) ? u->prefix_ops : 0;
}
double cfgpp_unet_device_bytes(cfgpp_unet* u) { return u ? u->dev_bytes : 0.0; }

// ---- LoRA: in-place merge into the repacked weights -------------------------------
// the slot of `key`, or null with the reason (naming the key) in the error string
static WeightSlot* lora_slot(cfgpp_unet* u, const char* key, const char* who) {
    if (!u || !key) { cfgpp_set_error("%s: null argument", who); return nullptr; }
    if (!u->finalized) { cfgpp_set_error("%s: %s: the engine is not finalized (weights are merged into the uploaded, repacked matrices)", who, key); return nullptr; }
    const std::string k = key;
    if (k == "conv_in.weight" || k == "conv_out.weight") {
        cfgpp_set_error("%s: %s runs on the fp32 small-kernel path and takes no adapter", who, key); return nullptr;
    }
    auto it = u->params.find(k);
    if (it == u->params.end()) { cfgpp_set_error("%s: unknown key %s", who, key); return nullptr; }
    if (!it->second.is_matrix) { cfgpp_set_error("%s: %s is a 1-D parameter (bias / norm): adapters apply to matrices", who, key); return nullptr; }
    auto sl = u->slots.find(k);
    if (sl == u->slots.end()) { cfgpp_set_error("%s: %s is not held as an fp16 matrix (fp32 direct-convolution path)", who, key); return nullptr; }
    return &sl->second;
}

int cfgpp_unet_lora(cfgpp_unet* u, const char* key, const float* up, const float* down, int rank, void* stream) {
    WeightSlot* w = lora_slot(u, key, "lora");
    if (!w) return -2;
    CFGPP_REQUIRE(rank >= 0, "lora: %s: rank %d", key, rank);
    CFGPP_REQUIRE(rank == 0 || (up && down), "lora: %s: rank %d with a null up / down matrix", key, rank);
    CFGPP_HIP_CHECK(hipSetDevice(u->device));
    hipStream_t s = (hipStream_t)stream;
    const size_t bytes = (size_t)w->O * w->K() * sizeof(half_t);
    if (rank == 0) {                        // restore; a parameter never merged into still is its base
        if (w->base) {
            CFGPP_HIP_CHECK(hipMemcpyAsync(w->rows(), w->base, bytes, hipMemcpyDeviceToDevice, s));
            return u->refold(w->rows(), s);     // (an upsampler conv in the 2x2 phase form reads a folded copy)
        }
        return 0;
    }
    if (!w->base) {                         // first merge into this parameter: keep what finalize uploaded (until destroy)
        half_t* b = (half_t*)u->dmalloc(bytes, false);
        CFGPP_REQUIRE(b, "lora: %s: out of device memory for the saved base (%zu bytes)", key, bytes);
        CFGPP_HIP_CHECK(hipMemcpyAsync(b, w->rows(), bytes, hipMemcpyDeviceToDevice, s));
        w->base = b;
    }
    const int kind = w->kind == SLOT_MEMBER ? SLOT_PLAIN : w->kind;
    int e = lora_merge_launch(w->base, w->rows(), up, down, rank, kind, w->O, w->I, w->taps, s);
    if (e) { const std::string m = cfgpp_last_error(); cfgpp_set_error("lora: %s: %s", key, m.c_str()); return e; }
    return u->refold(w->rows(), s);             // (an upsampler conv in the 2x2 phase form reads a folded copy)
}

// test / debugging hook (cfgpp_debug.h): the current weight of `key`, un-repacked to checkpoint order ([O][I][kh][kw] / [O][I])
int cfgpp_unet_read_weight(cfgpp_unet* u, const char* key, void* host_fp16_out) {
    WeightSlot* w = lora_slot(u, key, "read_weight");
    if (!w) return -2;
    CFGPP_REQUIRE(host_fp16_out, "read_weight: %s: null output", key);
    const long O = w->O, Kc = w->K(), I = w->I; const int taps = w->taps;
    std::vector<half_t> r((size_t)O * Kc);
    CFGPP_HIP_CHECK(hipSetDevice(u->device));
    CFGPP_HIP_CHECK(hipDeviceSynchronize());
    CFGPP_HIP_CHECK(hipMemcpy(r.data(), w->rows(), r.size() * sizeof(half_t), hipMemcpyDeviceToHost));
    half_t* out = (half_t*)host_fp16_out;
    for (long p = 0; p < O; ++p) {
        long o = p;
        if (w->kind == SLOT_GEGLU) { const long q = p & 63; o = (p >> 6) * 32 + (q & 31) + (q >= 32 ? O / 2 : 0); }
        const half_t* src = &r[(size_t)p * Kc];
        half_t* dst = out + (size_t)o * Kc;
        if (w->kind == SLOT_CONV3) {
            for (long i = 0; i < I; ++i) for (int t = 0; t < taps; ++t) dst[i * taps + t] = src[((i >> 6) * taps + t) * 64 + (i & 63)];
        } else {
            std::memcpy(dst, src, Kc * sizeof(half_t));
        }
    }
    return 0;
}

// ---- single-op wrappers for tests ----------------------------------------------
// test hook: the next cfgpp_op_igemm launches write GroupNorm statistics of their output (IGemmArgs::gstat) into `buf`
// ([M / 32][N][2] floats; null = off); cfgpp_op_igemm_gstat_written() = what the last launch reported through stat_flag
static float* g_op_gstat = nullptr;
static int g_op_gstat_flag = 0;
void cfgpp_op_igemm_set_gstat(void* buf) { g_op_gstat = (float*)buf; }
int cfgpp_op_igemm_gstat_written() { return g_op_gstat_flag; }

int cfgpp_op_igemm(const void* a0, const void* a1, int C0, int C1, int taps, int amode, int H, int W,
                   const void* w, int M, int N, const float* bias, const float* temb, int temb_ld,
                   const void* resid, int rmode, int rld, void* out, int omode, int old_, int epi, void* stream) {
    IGemmArgs a = base_args();
    a.a0 = (const half_t*)a0; a.a1 = (const half_t*)a1; a.C0 = C0; a.C1 = C1; a.taps = taps; a.amode = amode; a.H = H; a.W = W;
    a.w = (const half_t*)w; a.M = M; a.N = N; a.K = taps * (C0 + C1); a.bias = bias; a.temb = temb; a.temb_ld = temb_ld;
    a.rows_per_batch = H * W; a.resid = (const half_t*)resid; a.rmode = rmode; a.rld = rld;
    a.out = (half_t*)out; a.omode = omode; a.old = old_; a.epi = epi;
    a.gstat = g_op_gstat; a.stat_flag = &g_op_gstat_flag; g_op_gstat_flag = 0;
    return igemm_launch(a, (hipStream_t)stream);
}

// cfgpp_op_igemm plus the arguments it cannot pass: ashift (amode 2), out_scale and the tuner's cfg_hint
int cfgpp_op_igemm_ex(const void* a0, const void* a1, int C0, int C1, int taps, int amode, int H, int W,
                      const void* w, int M, int N, const float* bias, const float* temb, int temb_ld,
                      const void* resid, int rmode, int rld, void* out, int omode, int old_, int epi,
                      int ashift, float out_scale, int cfg_hint, void* stream) {
    IGemmArgs a = base_args();
    a.a0 = (const half_t*)a0; a.a1 = (const half_t*)a1; a.C0 = C0; a.C1 = C1; a.taps = taps; a.amode = amode; a.H = H; a.W = W;
    a.w = (const half_t*)w; a.M = M; a.N = N; a.K = taps * (C0 + C1); a.bias = bias; a.temb = temb; a.temb_ld = temb_ld;
    a.rows_per_batch = H * W; a.resid = (const half_t*)resid; a.rmode = rmode; a.rld = rld;
    a.out = (half_t*)out; a.omode = omode; a.old = old_; a.epi = epi;
    a.ashift = ashift; a.out_scale = out_scale; a.cfg_hint = cfg_hint;
    a.gstat = g_op_gstat; a.stat_flag = &g_op_gstat_flag; g_op_gstat_flag = 0;
    return igemm_launch(a, (hipStream_t)stream);
}

int cfgpp_op_fold_upsample(const void* w9, void* w4, int O, int I, void* stream) {
    return igemm_fold_upsample_launch((const half_t*)w9, (half_t*)w4, O, I, (hipStream_t)stream);
}

// nearest-2x upsample + conv3x3 as the plan builder emits it (Plan::conv3x3): the 2x2 phase form when upsample_phase_form says
// so, else the 9-tap launch
int cfgpp_op_upsample_conv3x3(const void* src, int C, int Hs, int Ws, const void* w9, const void* w4, int rows, int N,
                              const float* bias, void* out, void* stream) {
    IGemmArgs a = base_args();
    const bool ph = w4 != nullptr && upsample_phase_form(Hs, Ws, N);
    a.a0 = (const half_t*)src; a.C0 = C; a.taps = ph ? 4 : 9; a.amode = ph ? 4 : 3; a.H = 2 * Hs; a.W = 2 * Ws;
    a.w = (const half_t*)(ph ? w4 : w9); a.M = rows * a.H * a.W; a.N = N; a.K = a.taps * C; a.bias = bias;
    a.rows_per_batch = a.H * a.W; a.out = (half_t*)out; a.omode = 1; a.old = N; a.epi = EPI_STORE;
    a.gstat = g_op_gstat; a.stat_flag = &g_op_gstat_flag; g_op_gstat_flag = 0;
    return igemm_launch(a, (hipStream_t)stream);
}

int cfgpp_op_igemm_heads(const void* a_, int K, const void* w, int M, int N, const float* bias, int rows_per_batch,
                         void* hq, void* hk, void* hvt, int part0, int part_width, int head_dim, int heads,
                         int q_tok_pad, int tok_pad, void* stream) {
    IGemmArgs a = base_args();
    a.a0 = (const half_t*)a_; a.C0 = K; a.amode = 0; a.w = (const half_t*)w; a.M = M; a.N = N; a.K = K; a.bias = bias;
    a.epi = EPI_HEADS; a.rows_per_batch = rows_per_batch; a.hq = (half_t*)hq; a.hk = (half_t*)hk; a.hvt = (half_t*)hvt;
    a.part0 = part0; a.part_width = part_width; a.head_dim = head_dim; a.head_dim_pad = round_up(head_dim, 32);
    a.heads = heads; a.q_tok_pad = q_tok_pad; a.tok_pad = tok_pad;
    return igemm_launch(a, (hipStream_t)stream);
}

}  // extern "C"

// cfgpp_op_igemm_heads plus vt_linear (V^T columns in natural key order, as the VAE's attention consumes them)
int cfgpp_op_igemm_heads_ex(const void* a_, int K, const void* w, int M, int N, const float* bias, int rows_per_batch,
                            void* hq, void* hk, void* hvt, int part0, int part_width, int head_dim, int heads,
                            int q_tok_pad, int tok_pad, int vt_linear, void* stream) {
    IGemmArgs a = base_args();
    a.a0 = (const half_t*)a_; a.C0 = K; a.amode = 0; a.w = (const half_t*)w; a.M = M; a.N = N; a.K = K; a.bias = bias;
    a.epi = EPI_HEADS; a.rows_per_batch = rows_per_batch; a.hq = (half_t*)hq; a.hk = (half_t*)hk; a.hvt = (half_t*)hvt;
    a.part0 = part0; a.part_width = part_width; a.head_dim = head_dim; a.head_dim_pad = round_up(head_dim, 32);
    a.heads = heads; a.q_tok_pad = q_tok_pad; a.tok_pad = tok_pad; a.vt_linear = vt_linear ? 1 : 0;
    return igemm_launch(a, (hipStream_t)stream);
}
