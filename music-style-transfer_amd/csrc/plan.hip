// Plan builder + C ABI.  A plan is the whole StyleTransferModel (style/model.py:727-793) for one
// (layer widths, clip shape) unrolled into a static list of ops; every op carries its forward
// launch steps AND the backward steps that undo it, so loss.backward() is "walk the list in
// reverse".  All descriptors are uploaded once at plan creation; running a plan only enqueues
// kernels on the caller's stream (no allocation, no host sync => hipGraph-capturable).
//
// Workspace layout (floats):  [ activations | gradients (same offsets) | scratch ], each arena holding
// one slice per clip.  A plan for K clips (mst_dims.clips) is the one-clip plan with every launch
// widened: at schedule time each descriptor is replicated K times with its workspace / note-tensor
// offsets relocated to clip k's slices, so the launch count stays that of one clip while every
// launch carries K times the work.  Clips never mix: `combine`, the loss tree and the LSTM chains are
// per clip (B = 1 in the reference); only the parameter gradients are summed over clips, in order.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <array>
#include <vector>

#include "mst_common.h"

#define MST_ALIGN_UP(n) (((n) + 63) / 64 * 64)

// ------------------------------------------------------------------------------------------ sizes
static int mean_size(double a, double b, double factor = 1.0) { return (int)std::ceil(((a + b) / 2.0) * factor); }

Sizes mst_sizes(const mst_dims& d) {
    Sizes z{};
    z.I = d.instr; z.STYLE = d.style; z.BAR = d.bar; z.H = d.beat; z.HB = d.bar / 2; z.RH = d.rhythm;
    z.MEL = d.melody; z.NRF = d.nrf; z.NI = d.n_instruments;
    z.OC = mean_size(NF * NPF, d.beat);                       // style/model.py:41-42
    z.PCE_IL = mean_size(d.instr, d.beat);                    // :43
    z.SE_L = mean_size(d.bar, d.style);                       // :148-151
    z.SE_IL = mean_size(d.instr, d.style, .25);
    z.SE_ML = mean_size(2, d.style, .1);
    z.SE_BL = mean_size(d.style, 1, .05);
    z.ME_BL = mean_size(d.beat, d.melody);                    // :207-211
    z.ME_BRL = mean_size(d.bar, d.melody);
    z.ME_IL = mean_size(d.instr, d.melody, .25);
    z.ME_CW = mean_size(NPF, d.melody);
    z.PRE_BL = mean_size(d.beat, d.rhythm);                   // :305-311
    z.PRE_BRL = mean_size(d.bar, d.rhythm, .5);
    z.PRE_CL = mean_size(NPN * NPF, d.rhythm, .1);
    z.PRE_IL = mean_size(d.instr, d.rhythm, .5);
    z.PRE_ML = mean_size(2, d.rhythm, .25);
    z.PRE_BPL = mean_size(1, d.rhythm, .25);
    z.URE_CL = mean_size(NUN * NUF, d.rhythm, .25);           // :390-391
    z.SIM_BL = mean_size(NF * d.rhythm, d.nrf, .05);          // :450-460
    z.SIM_SI = mean_size(d.style, d.n_instruments, .05);
    z.SIM_RI = mean_size(d.rhythm, d.n_instruments, .25);
    z.SIM_SM = mean_size(d.style, 2, .01);
    z.SIM_RM = mean_size(d.rhythm, 2, .1);
    z.SIM_SB = mean_size(d.style, 1, .01);
    z.SIM_RB = mean_size(d.rhythm, 1, .1);
    z.PSA_SL = mean_size(d.style, NPF, .5);                   // :586-590
    z.PSA_RL = mean_size(d.rhythm, NPF, .5);
    z.PSA_IL = mean_size(d.instr, NPF, .4);
    z.PSA_ML = mean_size(d.melody, NPF, 3);
    z.USA_SL = mean_size(d.style, NUF, .5);                   // :682-684
    z.USA_RL = mean_size(d.rhythm, NUF, 1);
    return z;
}

// ------------------------------------------------------------------------------------------ params
struct PInfo { std::string name; int64_t off, numel; int ndim; int shape[3]; };

struct ParamTable {
    std::vector<PInfo> v;
    std::map<std::string, int> idx;
    int64_t top = 0;
    void add(const std::string& name, int a, int b = 0, int c = 0) {
        PInfo p; p.name = name; p.off = top; p.ndim = 1 + (b > 0) + (c > 0);
        p.shape[0] = a; p.shape[1] = b; p.shape[2] = c;
        p.numel = (int64_t)a * (b > 0 ? b : 1) * (c > 0 ? c : 1);
        top += p.numel;
        idx[name] = (int)v.size();
        v.push_back(p);
    }
    void lin(const std::string& pre, int out, int in) { add(pre + ".weight", out, in); add(pre + ".bias", out); }
    void lstm(const std::string& pre, int in, int hid, bool bi) {
        for (int r = 0; r < (bi ? 2 : 1); ++r) {
            const std::string sfx = r ? "_reverse" : "";
            add(pre + ".weight_ih_l0" + sfx, 4 * hid, in);
            add(pre + ".weight_hh_l0" + sfx, 4 * hid, hid);
            add(pre + ".bias_ih_l0" + sfx, 4 * hid);
            add(pre + ".bias_hh_l0" + sfx, 4 * hid);
        }
    }
    int64_t off(const std::string& name) const {
        auto it = idx.find(name);
        if (it == idx.end()) { fprintf(stderr, "mst: unknown parameter %s\n", name.c_str()); abort(); }
        return v[it->second].off;
    }
};

// registration order == model.parameters() order (style/model.py:737-749 and each ctor)
static void build_params(const mst_dims& d, const Sizes& z, ParamTable& t) {
    std::string m = "pitched_channels_encoder";
    t.add(m + ".beats_conv.module.weight", z.OC, NF * NPF, CONV_K);
    t.add(m + ".beats_conv.module.bias", z.OC);
    t.lin(m + ".instruments_linear", z.PCE_IL, z.I);
    t.lin(m + ".linear", z.H, z.OC * NOCT + z.PCE_IL);
    t.lstm(m + ".beats_lstm.module", z.H, z.H, false);
    t.lstm(m + ".bars_lstm", z.H, z.HB, true);
    m = "unpitched_channels_encoder";
    t.lin(m + ".linear", z.H, NF * NUN * NUF);
    t.lstm(m + ".beats_lstm.module", z.H, z.H, false);
    t.lstm(m + ".bars_lstm", z.H, z.HB, true);
    m = "style_encoder";
    t.lstm(m + ".bars_lstm", z.BAR, z.SE_L, false);
    t.lin(m + ".instruments_linear", z.SE_IL, z.I);
    t.lin(m + ".mode_linear", z.SE_ML, 2);
    t.lin(m + ".bpm_linear", z.SE_BL, 1);
    t.lin(m + ".linear", z.STYLE, z.SE_L + z.SE_IL + z.SE_ML + z.SE_BL);
    m = "melody_encoder";
    t.lin(m + ".beats_linear", z.ME_BL, z.H);
    t.lin(m + ".bars_linear", z.ME_BRL, z.BAR);
    t.lin(m + ".instruments_linear", z.ME_IL, z.I);
    t.lin(m + ".octave_linear", z.MEL * NOCT, z.ME_BL + z.ME_BRL + z.ME_IL);
    t.lin(m + ".scale_degree_linear", z.MEL * NDEG, z.ME_BL + z.ME_BRL + z.ME_IL);
    t.lin(m + ".channels_linear", z.ME_CW, NPF);
    t.lin(m + ".linear", z.MEL, z.MEL + z.ME_CW);
    m = "pitched_rhythm_encoder";
    t.lin(m + ".beats_linear", z.PRE_BL, z.H);
    t.lin(m + ".bars_linear", z.PRE_BRL, z.BAR);
    t.lin(m + ".channels_linear", z.PRE_CL, NPN * NPF);
    t.lin(m + ".instruments_linear", z.PRE_IL, z.I);
    t.lin(m + ".mode_linear", z.PRE_ML, 2);
    t.lin(m + ".bpm_linear", z.PRE_BPL, 1);
    t.lin(m + ".linear", z.RH, z.PRE_BL + z.PRE_BRL + z.PRE_CL + z.PRE_IL + z.PRE_ML + z.PRE_BPL);
    m = "unpitched_rhythm_encoder";
    t.lin(m + ".beats_linear", z.PRE_BL, z.H);
    t.lin(m + ".bars_linear", z.PRE_BRL, z.BAR);
    t.lin(m + ".channels_linear", z.URE_CL, NUN * NUF);
    t.lin(m + ".bpm_linear", z.PRE_BPL, 1);
    t.lin(m + ".linear", z.RH, z.PRE_BL + z.PRE_BRL + z.URE_CL + z.PRE_BPL);
    m = "song_info_model";
    t.lstm(m + ".beats_lstm.module", NF * z.RH, z.SIM_BL, false);
    t.lstm(m + ".bars_lstm", z.SIM_BL, z.NRF, false);
    t.lin(m + ".style_instruments_linear", z.SIM_SI, z.STYLE);
    t.lin(m + ".rhythm_instruments_linear", z.SIM_RI, z.NRF);
    t.lin(m + ".instruments_linear", z.NI, z.SIM_SI + z.SIM_RI);
    t.lin(m + ".style_mode_linear", z.SIM_SM, z.STYLE);
    t.lin(m + ".rhythm_mode_linear", z.SIM_RM, z.NRF);
    t.lin(m + ".mode_linear", 2, z.SIM_SM + z.SIM_RM);
    t.lin(m + ".style_bpm_linear", z.SIM_SB, z.STYLE);
    t.lin(m + ".rhythm_bpm_linear", z.SIM_RB, z.NRF);
    t.lin(m + ".bpm_linear", 1, z.SIM_SB + z.SIM_RB);
    m = "pitched_style_applier";
    t.lin(m + ".style_linear", z.PSA_SL, z.STYLE);
    t.lin(m + ".rhythm_linear", z.PSA_RL, z.RH);
    t.lin(m + ".instruments_linear", z.PSA_IL, z.I);
    t.lin(m + ".octave_linear", NPF * 6 * NOCT, z.PSA_SL + z.PSA_RL + z.PSA_IL);
    t.lin(m + ".scale_degree_linear", NPF * 6 * NDEG, z.PSA_SL + z.PSA_RL + z.PSA_IL);
    t.lin(m + ".melody_linear", z.PSA_ML, z.MEL);
    t.lin(m + ".linear", NPF, NPF * 6 + z.PSA_ML);
    m = "unpitched_style_applier";
    t.lin(m + ".style_linear", NF * z.USA_SL, z.STYLE);
    t.lin(m + ".rhythm_linear", z.USA_RL, z.RH);
    t.lin(m + ".notes_linear", NUN * NUF * 4, z.USA_SL + z.USA_RL);
    t.lin(m + ".linear", NUF, NUF * 4);
}

// The one width rule of mst_widths_supported and plan construction: the note kernels' melody widths, and the hidden size of
// each of the seven LSTMs (both channel encoders' beats / bars LSTMs, the style encoder's, the song-info beats / bars LSTMs)
static bool widths_supported(const Sizes& z) {
    for (const int h : {z.H, z.HB, z.SE_L, z.SIM_BL, z.NRF})
        if (!lstm_hidden_supported(h)) return false;
    return notes_widths_supported(z.MEL, z.ME_CW, z.PSA_ML);
}

static bool dims_ok(const mst_dims* d) {
    // C <= 24: the applier's backward kernel runs one wave per channel pair of a qf in ONE workgroup (LDS of 12 waves); a MIDI file
    // has 16 channels, so the reference's own inputs stop at 15 pitched channels
    return d && d->C >= 1 && d->C <= COMBINE_MAXC && d->C <= 24 && d->R >= 1 && d->T >= 1 && d->beat >= 1 && d->bar >= 2 &&
           d->bar % 2 == 0 && d->nrf >= 1 && d->style >= 1 && d->melody >= 1 && d->rhythm >= 1 && d->instr >= 1 &&
           d->n_instruments >= 1 && d->clips >= 0 && d->clips <= 4096;
}

extern "C" int32_t mst_param_count(const mst_dims* d) {
    if (!dims_ok(d)) return MST_ERR_ARG;
    ParamTable t; build_params(*d, mst_sizes(*d), t);
    return (int32_t)t.v.size();
}
extern "C" int64_t mst_param_floats(const mst_dims* d) {
    if (!dims_ok(d)) return MST_ERR_ARG;
    ParamTable t; build_params(*d, mst_sizes(*d), t);
    return t.top;
}
extern "C" int32_t mst_param_info(const mst_dims* d, int32_t i, char* name, int32_t cap, int64_t* off, int32_t* ndim,
                                  int32_t shape[3]) {
    if (!dims_ok(d) || !name || !off || !ndim || !shape) return MST_ERR_ARG;
    ParamTable t; build_params(*d, mst_sizes(*d), t);
    if (i < 0 || i >= (int)t.v.size()) return MST_ERR_ARG;
    const PInfo& p = t.v[i];
    snprintf(name, cap, "%s", p.name.c_str());
    *off = p.off; *ndim = p.ndim;
    for (int k = 0; k < 3; ++k) shape[k] = p.shape[k];
    return MST_OK;
}

// ------------------------------------------------------------------------------------------ plan
struct T { int64_t off; int rows, cols, ld; };
struct SegIn { int space; int64_t off; int ld, width; int s[4]; bool grad; };
enum { K_GEMM, K_GATHER, K_SEGRED, K_LSTM_F, K_LSTM_B, K_COMB_F, K_COMB_B, K_ME_F, K_ME_B, K_PSA_F, K_PSA_B, K_LSTM_T, K_ROW_F, K_ROW_B,
       K_ME_SQ, K_ME_RED,
       // tiled plans only (never merged): halves of a combine, strided copies, fold / spread around an exchange, the exchange
       K_COMB_F1, K_COMB_F2, K_COMB_B1, K_COMB_B2, K_COPY_F, K_COPY_B, K_FOLD, K_SPREAD, K_XCHG,
       K_GEMM_FOLD,        // weight-gradient GEMMs of a batched plan with the clips folded into K (one descriptor for all clips)
       K_CONV_P, K_CONV_F, K_CONV_W,    // batched plans on the 64x64 tiling: the note-axis convolution on its own kernels (conv.hip)
       K_LIN_F, K_LIN_A, K_LIN_W,       // ... and its large dense nn.Linear layers (lin.hip): forward, input gradient, weight gradient
       K_COUNT };
// Per step kind (the values above are ABI: bench.py and the tests name them): the descriptor family Step.first indexes; sched:
// in a scheduled list it indexes the family's scheduled (per-clip relocated) descriptors, not the build-time ones; per_clip: the
// scheduler replicates the step per clip (K_GEMM_FOLD: one descriptor for all clips); merge: same-level steps may share a launch.
enum { F_GEMM, F_GATHER, F_SEGRED, F_LSTM, F_COMB, F_NOTES, F_ROWLIN, F_COPY, F_FOLD, F_XCHG, F_CONV, F_LIN };
struct KindInfo { int kind, fam, sched, per_clip, merge; };
static constexpr KindInfo KINDS[] = {
    {K_GEMM, F_GEMM, 1, 1, 1},     {K_GATHER, F_GATHER, 1, 1, 1}, {K_SEGRED, F_SEGRED, 1, 1, 1}, {K_LSTM_F, F_LSTM, 1, 1, 1},
    {K_LSTM_B, F_LSTM, 1, 1, 1},   {K_COMB_F, F_COMB, 1, 1, 1},   {K_COMB_B, F_COMB, 1, 1, 1},   {K_ME_F, F_NOTES, 1, 1, 0},
    {K_ME_B, F_NOTES, 1, 1, 0},    {K_PSA_F, F_NOTES, 1, 1, 0},   {K_PSA_B, F_NOTES, 1, 1, 0},   {K_LSTM_T, F_LSTM, 1, 1, 1},
    {K_ROW_F, F_ROWLIN, 1, 1, 0},  {K_ROW_B, F_ROWLIN, 1, 1, 0},  {K_ME_SQ, F_NOTES, 1, 1, 0},   {K_ME_RED, F_NOTES, 1, 1, 0},
    {K_COMB_F1, F_COMB, 1, 1, 0},  {K_COMB_F2, F_COMB, 1, 1, 0},  {K_COMB_B1, F_COMB, 1, 1, 0},  {K_COMB_B2, F_COMB, 1, 1, 0},
    {K_COPY_F, F_COPY, 0, 0, 0},   {K_COPY_B, F_COPY, 0, 0, 0},   {K_FOLD, F_FOLD, 0, 0, 0},     {K_SPREAD, F_FOLD, 0, 0, 0},
    {K_XCHG, F_XCHG, 0, 0, 0},     {K_GEMM_FOLD, F_GEMM, 1, 0, 1}, {K_CONV_P, F_CONV, 0, 0, 0},  {K_CONV_F, F_CONV, 0, 0, 0},
    {K_CONV_W, F_CONV, 0, 0, 0},   {K_LIN_F, F_LIN, 0, 0, 0},     {K_LIN_A, F_LIN, 0, 0, 0},     {K_LIN_W, F_LIN, 0, 0, 0}};
static constexpr bool kinds_in_order(int i = 0) { return i == K_COUNT || (KINDS[i].kind == i && kinds_in_order(i + 1)); }
static_assert(sizeof(KINDS) / sizeof(KINDS[0]) == K_COUNT && kinds_in_order(), "KINDS[k] describes step kind k, for every k");

template <class D>
static int up(const std::vector<D>& v, D** dev) {
    *dev = nullptr;
    if (v.empty()) return 0;
    if (hipMalloc((void**)dev, v.size() * sizeof(D)) != hipSuccess) return MST_ERR_ALLOC;
    if (hipMemcpy(*dev, v.data(), v.size() * sizeof(D), hipMemcpyHostToDevice) != hipSuccess) return MST_ERR_ALLOC;
    return 0;
}
// One descriptor family: as built (one clip), as scheduled (replicated families: per clip, relocated, in launch order) and on
// the device — the scheduled copies, or the built ones for a family the scheduler never replicates (its `sched` stays empty).
template <class D> struct DescTable {
    std::vector<D> host, sched;
    D* dev = nullptr;
    int upload() { return up(sched.empty() ? host : sched, &dev); }
    void release() { hipFree(dev); dev = nullptr; }
};

// What a K_GEMM launch can carry besides its members (mst_plan::mixes), one step of its level per slot, in the order of their
// blocks in the launch: the K_LSTM_B step of hidden sizes <= LSTM_RIDE_H, the K_COMB_F / K_COMB_B step of small sites, the one of
// large sites (whose second phase is a launch behind the carrier), the K_SEGRED step (its first stage) and the K_GATHER step
enum { RIDE_LSTM, RIDE_COMB_SMALL, RIDE_COMB_LARGE, RIDE_SEGRED, RIDE_GATHER, RIDE_SLOTS };
struct Step { int kind, first, count, a, b, stage; int c = 0; int lvl = 0; int chain = -1; int signal = -1; int wait[3] = {-1, -1, -1};
              int carrier = -1; int rider[RIDE_SLOTS] = {-1, -1, -1, -1, -1}; };
// c: GEMM steps — offset of the step's block -> member table; lvl: dependency level in its scheduled pass; chain / signal / wait: the stream the
// launch goes to, the event slot recorded behind it and the slots its stream waits for in front of it (assign_streams; chain -1 = caller's stream)
// carrier: index, in its scheduled list, of the K_GEMM step whose launch runs this step (-1: its own launch).  A carried step stays in the
// list (dependencies, first-writer flags, instrumentation); its carrier's rider[slot] is its index, and run_step reads its descriptors
// (first, count / clips, a, b) from the carried step itself.  Indices, not pointers: the lists are vectors of values
// a second stage that stays a launch of its own, directly behind the launch that ran the first: a two-stage segment reduce, a combine of large sites
static bool second_stage(const Step& s) { return (s.kind == K_SEGRED && s.b > 0) || ((s.kind == K_COMB_F || s.kind == K_COMB_B) && s.b != 0); }
struct Acc { int space; int64_t lo, hi; bool w; bool accum = false, dense = true; };   // accum: a += writer; dense: covers [lo, hi) fully
struct Op { int stage; std::vector<Step> fwd, bwd; };

static int stage_idx(int stage) { return stage == MST_STAGE_EXTRACT ? 0 : stage == MST_STAGE_INFO ? 1 : 2; }

struct mst_plan {
    mst_dims d; Sizes z; ParamTable pt;
    DescTable<GemmDesc> gemms; DescTable<GatherDesc> gathers; DescTable<SegRedDesc> segreds; DescTable<LstmDesc> lstms;
    DescTable<CombineDesc> combines; DescTable<NotesDesc> notes; DescTable<RowLinDesc> rowlins;
    DescTable<ConvDesc> convs; DescTable<LinDesc> lins; DescTable<CopyDesc> copies; DescTable<FoldDesc> folds;
    std::vector<SlabEntry> slabs[3];
    std::vector<Op> ops;
    // scheduled launch lists (dependency-levelled, same-level steps merged) and their descriptor arrays
    std::vector<Step> sched[2];        // per-stage merging (stages may run separately)
    std::vector<Step> sched_all[2];    // stage-agnostic merging, used when all stages run together
    const std::vector<Step>& list(int mask, int backward) const { return mask == MST_STAGE_ALL ? sched_all[backward ? 1 : 0] : sched[backward ? 1 : 0]; }
    // member of every workgroup of a clip's block range, per scheduled GEMM launch (Step.c): one uniform load instead of a binary
    // search over the members' first blocks — log2(members) dependent scalar round trips at the head of every workgroup
    std::vector<int> s_gemm_owner; int* d_gemm_owner = nullptr;
    std::map<std::string, T> named;
    int64_t act_top = 0, tmp_top = 0;
    SlabEntry* d_slabs[3] = {nullptr, nullptr, nullptr};
    std::vector<SlabBlock> slab_blocks[3]; SlabBlock* d_slab_blocks[3] = {nullptr, nullptr, nullptr};
    // all three stages' entries as ONE launch (a whole-model backward): valid when no parameter range is the target of two entries
    std::vector<SlabEntry> slabs_all; SlabEntry* d_slabs_all = nullptr;
    std::vector<SlabBlock> slab_blocks_all; SlabBlock* d_slab_blocks_all = nullptr;
    bool slabs_all_ok = false;
    T t_losses, t_saved, t_gl; int64_t loss_scratch = 0;
    // clip 0's workspace offsets of what the loss kernels read and write (the gradient of a prediction: the same offset of SP_GRAD)
    // and the cells of a clip's note tensors; resolved once, where `named` is final.  up: only with an unpitched part
    struct LossOps { int64_t pp, up, il, mlg, bp, it, mt, bt, losses, saved, gl, np, nu; } loss{};
    void resolve_loss() {
        auto at = [&](const char* n) { return named.at(n).off; };
        const bool U = d.has_unpitched != 0;
        loss = {at("pitched_pred"), U ? at("unpitched_pred") : 0, at("instruments_pred"), at("mode_pred"), at("bpm_pred"),
                at("used_instruments"), at("mode"), at("bpm_target"), t_losses.off, t_saved.off, t_gl.off,
                (int64_t)P() * NF * NPN, U ? (int64_t)Q() * NF * NUN : 0};
    }
    std::vector<ZeroChunk> zero_stage[3], zero_all;      // gradient ranges mst_zero_grads clears (clip 0 coordinates)
    ZeroChunk* d_zero_stage[3] = {nullptr, nullptr, nullptr}; ZeroChunk* d_zero_all = nullptr;
    int err = 0;
    mst_plan_options opt{};       // as given to mst_plan_create_ex (zeros = defaults)
    int mfma = 0;                 // GEMM tiling of this plan: 1 = 64x64 tiles (batched, FLOP-bound plans), 0 = 32x32 split-K tiles (latency)
    int lstm_small_on = 1;        // H <= 16 LSTM launches take the one-wave kernels (mst_plan_set_lstm_small; 0: the register flavour)

    // bar tiling (mst_plan_options.tile_rows > 0): this rank owns bars [tile_r0, tile_r0 + tile_rows) of the d.R bars
    bool tiled() const { return opt.tile_rows > 0; }
    // a level's gathers and segment reduces ride on its GEMM launch: the one-stream, merged plans on the 32x32 tiling only
    bool mixes() const { return !mfma && !tiled() && opt.branches != 1 && !opt.no_merge; }
    // the combine kernels' compile-time channel bound: 4 where no site can have more channels, COMBINE_MAXC otherwise
    int mc4() const { return d.C <= 4 ? 1 : 0; }
    int Rl() const { return tiled() ? opt.tile_rows : d.R; }
    int P() const { return d.C * Rl() * d.T; }          // positions / beats this plan computes (all of them when not tiled)
    int Q() const { return Rl() * d.T; }
    struct Xchg { int space; int64_t off; int32_t len; };
    std::vector<Xchg> xchgs;
    bool tags_in_zero = false;             // zero_all also clears the multi-workgroup LSTM's exchange tags
    // step of sched_all[0] whose launch clears zero_all in mst_train_iteration (-1: mst_zero_grads is launched): the pass's first
    // launch, if it is a K_GEMM step that carries riders and neither it nor a step it carries touches a zero chunk
    int zero_ride = -1;
    void find_zero_ride();
    std::vector<ZeroChunk> zero_fwd; ZeroChunk* d_zero_fwd = nullptr;      // activation ranges cleared before a tiled forward
    int64_t loss_sum_off = 0;                                               // [SP_TMP] 16 floats: the loss partial sums, folded
    int loss_fold[2] = {-1, -1};
    // one train iteration of a tiled plan as phases: each runs launch steps and ends at an exchange (or at the end)
    // what: 0 schedule steps, 1 loss partials, 2 loss tail + seed; xchg[0 .. nx): the exchanges the phase ends at — exchanges of
    // one dependency level are MERGED into one phase end (what runs between them in the level-ordered list cannot depend on them)
    struct Phase { int what; int pass; int begin, end; int nx; int xchg[MST_MAX_XCHG]; };
    std::vector<Phase> phases;
    int K() const { return d.clips > 1 ? d.clips : 1; }
    static int device_cus() {          // compute units of the current device (256 on MI355X in SPX mode)
#ifdef HIPSIM
        return 16;                     // the interpreter co-schedules at most 48 blocks (hipsim::COOP_MAXB): 3 slots x 16
#else
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
        return cus;
#endif
    }
    // Workgroups of ONE launch of the multi-workgroup LSTM kernels that are certainly resident together on this device: what the
    // occupancy API reports per CU for these kernels minus one slot per CU, times the CUs.  The spare slot is the room for
    // whatever else is running (a second stream's kernel, an RCCL kernel, the tail of the previous launch); a launch that needs
    // more takes the single-workgroup flavour.  On a whole MI355X: (4 - 1) x 256 = 768 workgroups = 64 clips.
    static int coresident_slots() {
        const int per_cu = lstm_multi_blocks_per_cu();
        return per_cu > 1 ? (per_cu - 1) * device_cus() : 0;
    }
    int64_t status_off = 0;            // [SP_WS, clip 0] device status word ("device_status")
    // side streams of run_pass (mst_plan_options.branches): same-level launches fork from / join to the caller's stream
    // The launches of such plans' whole-model lists are spread over 1 + N_SIDE streams along the dependency DAG (assign_streams);
    // a set of side streams / events belongs to ONE caller stream (two accumulation iterations captured side by side must not
    // meet in a shared side stream), created at the caller's first (eager) pass.
    enum { N_SIDE = 3, N_SETS = 4, N_EVENTS = 96 };
    struct SideSet { hipStream_t owner = nullptr; bool used = false; hipStream_t side[N_SIDE] = {}; hipEvent_t ev_fork = nullptr, ev_join[N_SIDE] = {}, ev[N_EVENTS] = {}; };
    mutable SideSet sides[N_SETS];
    bool branches = false;
    SideSet* side_set(hipStream_t main) const {
        for (SideSet& q : sides) if (q.used && q.owner == main) return &q;
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(main, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return nullptr;      // no object creation inside a capture
        for (SideSet& q : sides) {
            if (q.used) continue;
            bool ok = hipEventCreateWithFlags(&q.ev_fork, hipEventDisableTiming) == hipSuccess;
            for (int i = 0; i < N_SIDE; ++i)
                ok = ok && hipStreamCreateWithFlags(&q.side[i], hipStreamNonBlocking) == hipSuccess &&
                     hipEventCreateWithFlags(&q.ev_join[i], hipEventDisableTiming) == hipSuccess;
            for (int i = 0; i < n_signals; ++i) ok = ok && hipEventCreateWithFlags(&q.ev[i], hipEventDisableTiming) == hipSuccess;
            if (!ok) return nullptr;
            q.used = true; q.owner = main;
            return &q;
        }
        return nullptr;                 // more caller streams than sets: that caller runs its chains back to back
    }
    int64_t ext0_stride() const { return (int64_t)P() * NF * NPN * NPF; }
    int64_t ext1_stride() const { return (int64_t)Q() * NF * NUN * NUF; }
    // float offset of an arena from the start of the workspace: every clip's activations, then their gradients, then the scratch
    // (-1: parameters and the borrowed inputs are not in the workspace)
    int64_t arena(int space) const {
        return space == SP_WS ? 0 : space == SP_GRAD ? (int64_t)K() * act_top : space == SP_TMP ? 2 * (int64_t)K() * act_top : -1;
    }
    LossBatch loss_batch() const { return {K(), act_top, act_top, tmp_top, ext0_stride(), ext1_stride()}; }      // the clips' strides
    // offset of clip k's slice of `space` relative to clip 0's
    int64_t shift(int space, int k) const {
        switch (space) {
        case SP_WS: case SP_GRAD: return (int64_t)k * act_top;
        case SP_TMP: return (int64_t)k * tmp_top;
        case SP_EXT0: return (int64_t)k * ext0_stride();
        case SP_EXT1: return (int64_t)k * ext1_stride();
        default: return 0;                                  // parameters are shared
        }
    }
    GemmDesc reloc(GemmDesc g, int k) const {
        for (Operand* o : {&g.A, &g.B}) {
            o->off += shift(o->space, k);
            if (o->kind == OPK_ACTGRAD || o->kind == OPK_CONVGRAD) o->off2 += shift(o->space2, k);
        }
        g.out.off += shift(g.out.space, k);
        if (g.out.bias_space >= 0) g.out.bias_off += shift(g.out.bias_space, k);      // 0 for a parameter bias
        return g;
    }
    GatherDesc reloc(GatherDesc g, int k) const {
        g.out_off += shift(SP_WS, k);
        for (int i = 0; i < g.nseg; ++i) g.seg[i].off += shift(g.seg[i].space, k);
        return g;
    }
    SegRedDesc reloc(SegRedDesc r, int k) const {
        r.src_off += shift(SP_GRAD, k); r.dst_off += shift(SP_GRAD, k); r.part_off += shift(SP_TMP, k); r.y_off += shift(SP_WS, k);
        return r;
    }
    LstmDesc reloc(LstmDesc l, int k) const {           // whht (W_hh transposed) is shared: parameters only
        const int64_t a = shift(SP_WS, k), t = shift(SP_TMP, k);
        l.zx_off += a; l.out_off += a; l.gout_off += a; l.gzx_off += a;
        l.gates_off += t; l.c_off += t; l.hprev_off += t; l.tc_off += t; l.xch_off += t;
        return l;
    }
    CombineDesc reloc(CombineDesc c, int k) const {
        const int64_t a = shift(SP_WS, k), t = shift(SP_TMP, k);
        c.x_off += a; c.out_off += a; c.gx_off += a; c.gout_off += a; c.stats_off += t; c.part_off += t;
        return c;
    }
    RowLinDesc reloc(RowLinDesc r, int k) const {
        r.x_off += shift(SP_WS, k); r.y_off += shift(SP_WS, k); r.slab_off += shift(SP_TMP, k);
        return r;
    }
    NotesDesc reloc(NotesDesc n, int k) const {
        const int64_t a = shift(SP_WS, k), t = shift(SP_TMP, k);
        n.oct_off += a; n.deg_off += a; n.rt_oct_off += a; n.rt_deg_off += a; n.it_oct_off += a; n.it_deg_off += a; n.mel_off += a; n.g_mel_off += a; n.out_off += a; n.g_out_off += a; n.g_oct_off += a; n.g_deg_off += a;
        n.g_ml_off += a; n.x_off += shift(n.x_space, k); n.slab_off += t; n.part_off += t; n.stats_off += t;
        n.itp_oct_off += a; n.itp_deg_off += a; n.loss_saved_off += a; n.loss_gl_off += a;
        return n;
    }
    // f(table) for a family the scheduler replicates (KINDS[k].sched)
    template <class F> void with_sched_table(int fam, F&& f) {
        switch (fam) {
        case F_GEMM: f(gemms); break;       case F_GATHER: f(gathers); break;     case F_SEGRED: f(segreds); break;
        case F_LSTM: f(lstms); break;       case F_COMB: f(combines); break;      case F_NOTES: f(notes); break;
        case F_ROWLIN: f(rowlins); break;   default: err = MST_ERR_UNSUPPORTED;
        }
    }

    static int64_t align(int64_t n) { return (n + 63) / 64 * 64; }
    T newT(int rows, int cols, const char* name = nullptr) {
        T t{act_top, rows, cols, cols};
        act_top += align((int64_t)rows * cols);
        if (name) named[name] = t;
        return t;
    }
    int64_t tmp(int64_t n) { int64_t o = tmp_top; tmp_top += align(n); return o; }
    static int tiles(int M, int N) { return ((M + GEMM_BM - 1) / GEMM_BM) * ((N + GEMM_BN - 1) / GEMM_BN); }
    // weight-gradient GEMMs reduce over rows.  One clip per launch (latency-bound): one k-split per 256 rows (2 k-tiles),
    // capped at 64 slabs, for workgroup count.  Batched plans get their parallelism from the clips, so a split covers
    // up to 2048 rows (64 MFMA k-tiles, at 64 clips) and the slab traffic of the deferred reduction shrinks accordingly.
    // batched plans on the 64x64 tiling fold the clips into the reduction of their weight-gradient GEMMs (GemmDesc.fold_rows)
    bool mfma_plan() const { return opt.gemm_tile == 64 || (opt.gemm_tile == 0 && K() >= 6); }      // the throughput GEMM tiling
    bool folds_clips() const { return K() > 1 && mfma_plan(); }
    // k-splits of a folded reduction: enough (tile, split) workgroups to fill every workgroup slot of the chip once (256 CUs x 4), at least
    // 128 reduction rows per split; the slab a split writes is one weight gradient, so many splits of a small weight are cheap
    int fold_splits(int rows, int M, int N, int members) const {
        const int64_t kt = (int64_t)rows * K();
        const int64_t t = (int64_t)((M + 63) / 64) * ((N + 63) / 64) * members;      // `members` like GEMMs share the launch
        int64_t s = 1024 / t;                // rounded DOWN: 1025 workgroups are two rounds of the chip
        const int64_t kmax = kt / 128;
        if (s > kmax) s = kmax;
        while (s > 1 && (int64_t)M * N * s > (int64_t)4 << 20) --s;      // <= 16 MB of slab per weight
        s = s < 1 ? 1 : (s > 512 ? 512 : s);
        const int64_t chunk = ((kt + s - 1) / s + 31) / 32 * 32;          // the kernel rounds a split's share to whole k-tiles:
        return (int)((kt + chunk - 1) / chunk);                           // no split may come out empty (its slab would stay unwritten)
    }
    // turns the weight-gradient GEMM `w` (built for one clip, reduction over `rows`) into the folded form
    void fold(GemmDesc& w, int rows, int members = 1) {
        w.fold_rows = rows; w.K = rows * K(); w.ksplit = fold_splits(rows, w.M, w.N, members);       // the clip strides are set at schedule time
    }
    int splits_for(int rows) const {
        const int per = 32 * K() < 256 ? 256 : (32 * K() > 2048 ? 2048 : 32 * K());
        int s = (rows + per - 1) / per;
        return s < 1 ? 1 : (s > 64 ? 64 : s);
    }

    // GEMM operands: a dense matrix (element (i, j) at off + i * si + j * sj); dY o act'(Y) of the output Y at `off` (transposed: j
    // runs along Y's rows)
    static Operand dense(int space, int64_t off, int64_t si, int64_t sj, int kfast, int ones_at = -1) {
        Operand o{}; o.kind = OPK_DENSE; o.space = space; o.off = off; o.si = si; o.sj = sj; o.ones_at = ones_at; o.kfast = kfast;
        return o;
    }
    static Operand actgrad(int64_t off, int ld, int act, bool transposed) {
        Operand o{}; o.kind = OPK_ACTGRAD; o.space = SP_GRAD; o.off = off; o.space2 = SP_WS; o.off2 = off;
        o.ld = ld; o.act = act; o.transposed = transposed ? 1 : 0; o.kfast = transposed ? 0 : 1;
        return o;
    }
    // slab entries that reduce `splits` slabs (M x wcols weights, then M biases) into the weight gradient at woff (dst_ld > 0: a
    // column block of a dst_ld-wide matrix at `base`) and the bias gradient at boff (none when < 0); single: one slab set for all clips
    void weight_slabs(int stage, int64_t woff, int64_t boff, int64_t slab, int64_t stride, int M, int wcols, int splits, bool single,
                      int dst_ld = 0, int64_t base = 0) {
        SlabEntry e{woff, slab, stride, M * wcols, splits}, eb{boff, slab + (int64_t)M * wcols, stride, M, splits};
        if (dst_ld) { e.width = wcols; e.dst_ld = dst_ld; e.base = base; }
        e.single = eb.single = single ? 1 : 0;
        slabs[stage_idx(stage)].push_back(e);
        if (boff >= 0) slabs[stage_idx(stage)].push_back(eb);
    }
    // weight-gradient tail: `w` (M, operands, out.pb / pc set) over `rows` rows of one clip -> M x wcols weights (+ a bias column
    // when boff >= 0), a k-split GEMM into a fresh slab, folded when may_fold on a plan that folds (`members` like GEMMs share its
    // launch), and its slab entries.  Pushes the GEMM, returns its launch step
    Step wgrad(int stage, GemmDesc w, int rows, int wcols, int64_t woff, int64_t boff, bool may_fold = true, int members = 1,
               int dst_ld = 0, int64_t base = 0) {
        w.N = wcols + (boff >= 0 ? 1 : 0); w.K = rows; w.ksplit = splits_for(rows);
        const bool fd = may_fold && folds_clips();
        if (fd) fold(w, rows, members);
        const int64_t stride = (int64_t)w.M * wcols + w.M;
        const int64_t slab = tmp(stride * w.ksplit);
        w.out.kind = w.out.pb ? OUT_PERMW_SLAB : OUT_SLAB; w.out.space = SP_TMP; w.out.off = slab; w.out.slab_stride = stride;
        w.out.wcols = wcols; w.out.bias_space = -1;
        const Step st{fd ? K_GEMM_FOLD : K_GEMM, (int)gemms.host.size(), 1, tiles(w.M, w.N), w.ksplit};
        gemms.host.push_back(w);
        weight_slabs(stage, woff, boff, slab, stride, w.M, wcols, w.ksplit, fd, dst_ld, base);
        return st;
    }
    // segment reduce of `nred` rows per output: one chunk per 64 rows; several chunks leave partial sums in scratch for a second
    // launch, whose workgroup count is returned (0: none)
    int partials(SegRedDesc& r, int nred) {
        r.nchunk = (nred + 63) / 64;
        if (r.nchunk <= 1) return 0;
        r.part_off = tmp((int64_t)r.nidx * r.nchunk * r.width);
        return (r.nidx * r.width + 255) / 256;
    }

    static SegIn seg(const T& t, int s0, int s1, int s2, int s3, bool grad = true) {
        return SegIn{SP_WS, t.off, t.ld, t.cols, {s0, s1, s2, s3}, grad};
    }

    // cat_with_broadcast (style/utils/pytorch.py:54-65) of several sources, materialised once.
    // forward: gather kernel; backward: segment-reduce of the concat's gradient into each source.
    // sum = true: the segments (equal widths) are added instead of concatenated — out = sum of the broadcast sources
    T gather(int stage, const int rs[4], const std::vector<SegIn>& segs, bool sum = false) {
        if (segs.size() > MAX_SEG) err = MST_ERR_UNSUPPORTED;
        const int rows = rs[0] * rs[1] * rs[2] * rs[3];
        int K = 0;
        for (auto& s : segs) { if (sum) { if (K && K != s.width) err = MST_ERR_UNSUPPORTED; K = s.width; } else K += s.width; }
        T out = newT(rows, K);
        GatherDesc g{}; g.rows = rows; g.K = K; g.nseg = (int)segs.size(); g.out_off = out.off; g.sum = sum ? 1 : 0;
        for (int q = 0; q < 4; ++q) g.d[q] = rs[q];
        int start = 0;
        for (size_t i = 0; i < segs.size(); ++i) {
            Seg& s = g.seg[i];
            s.space = segs[i].space; s.off = segs[i].off; s.ld = segs[i].ld; s.start = start; s.width = segs[i].width;
            for (int q = 0; q < 4; ++q) s.s[q] = segs[i].s[q];
            if (!sum) start += segs[i].width;
        }
        Op op; op.stage = stage;
        op.fwd.push_back(Step{K_GATHER, (int)gathers.host.size(), 1, rows, 0});
        gathers.host.push_back(g);
        int first = (int)segreds.host.size(), cnt = 0, maxidx = 1, stage2 = 0;
        start = 0;
        for (auto& s : segs) {
            if (s.grad) {
                SegRedDesc r{}; r.src_off = out.off; r.src_ld = K; r.start = start; r.width = s.width;
                r.dst_off = s.off; r.dst_ld = s.ld; r.nidx = 1;
                for (int q = 0; q < 4; ++q) {
                    r.d[q] = rs[q]; r.s[q] = s.s[q];
                    r.kd[q] = (s.s[q] != 0 && rs[q] > 1) ? rs[q] : 1;
                    r.nidx *= r.kd[q];
                }
                // destination rows must be the natural row-major index of the kept dims
                int nat = 1;
                for (int q = 3; q >= 0; --q) {
                    if (r.kd[q] > 1) { if (s.s[q] != nat) err = MST_ERR_UNSUPPORTED; nat *= r.kd[q]; }
                }
                int nred = 1;
                for (int q = 0; q < 4; ++q) if (r.kd[q] == 1) nred *= rs[q];
                stage2 = std::max(stage2, partials(r, nred));
                if (r.nidx * r.nchunk > maxidx) maxidx = r.nidx * r.nchunk;
                segreds.host.push_back(r); ++cnt;
            }
            if (!sum) start += s.width;
        }
        if (cnt) op.bwd.push_back(Step{K_SEGRED, first, cnt, maxidx, stage2});
        ops.push_back(op);
        return out;
    }

    // nn.Linear (+ activation) on a dense (rows x K, row stride ld) input that lives in `space`.
    // Emits the forward GEMM, the k-split weight|bias-gradient GEMM and, when the input needs a
    // gradient, the input-gradient GEMM accumulating straight into the input's gradient slot.
    T linear(int stage, int space, int64_t xoff, int xld, int rows, int K, bool xgrad, const std::string& wname,
             const std::string& bname, int N, int act, const T* out_opt = nullptr, int pb = 0, int pc = 0,
             const char* name = nullptr) {
        T out = out_opt ? *out_opt : newT(rows, N, name);
        const int64_t woff = pt.off(wname), boff = pt.off(bname);
        Op op; op.stage = stage;
        // Plans on the throughput tiling run their large dense Linears on lin.hip's kernels (2 x 2-blocked MFMA tiles, all clips
        // as rows of one launch): row-major input in the workspace or a borrowed note tensor, >= 512 rows and >= 4 MFLOP per clip
        // and more than one 32-column MFMA block of outputs — or at most 16 outputs of a long input row (the 16x16x4 stream kernels).  The rule does not look at the clip count: a one-clip plan forced
        // onto this tiling takes the same kernels, so "batched == one clip at a time, bit for bit" holds by construction.
        if (mfma_plan() && opt.dense_flavour != 1 && !pb && rows >= 32 && K >= 4 && N >= 4 && (space == SP_WS || ((space == SP_EXT0 || space == SP_EXT1) && !xgrad)) &&
            boff == woff + (int64_t)N * K && (int64_t)this->K() * rows < ((int64_t)1 << 30) &&
            (opt.dense_flavour == 2 || (rows >= 512 && N > 32 && 2.0 * rows * N * K >= 4e6) ||
             (rows >= 512 && N <= 16 && K >= 128 && K + 1 <= 320 && !xgrad))) {       // the N <= 16 stream kernels: 280 -> 16 over every note row
            LinDesc l{}; l.rows = rows; l.K = K; l.N = N; l.act = act; l.xgrad = xgrad ? 1 : 0; l.clips = this->K();
            l.x_space = space; l.x_ld = xld; l.x_off = xoff; l.y_ld = out.ld; l.y_off = out.off; l.w_off = woff; l.b_off = boff;
            const int64_t mtot = (int64_t)this->K() * rows;
            const int tl = lin_dw_tiles(l);
            int64_t sp = std::max<int64_t>(1, 768 / tl);       // three workgroups per CU, all co-resident
            int64_t per = ((mtot + sp - 1) / sp + 31) / 32 * 32;
            if (per < 128) per = 128;
            l.rows_per_split = per; l.splits = (int)((mtot + per - 1) / per);
            l.slab_stride = (int64_t)N * K + N;
            l.slab_off = tmp(l.slab_stride * l.splits);
            const int li = (int)lins.host.size();
            lins.host.push_back(l);
            op.fwd.push_back(Step{K_LIN_F, li, 1, 0, 0});
            op.bwd.push_back(Step{K_LIN_W, li, 1, 0, 0});
            if (xgrad) op.bwd.push_back(Step{K_LIN_A, li, 1, 0, 0});
            weight_slabs(stage, woff, boff, l.slab_off, l.slab_stride, N, K, l.splits, true);
            ops.push_back(op);
            return out;
        }
        GemmDesc g{}; g.M = rows; g.N = N; g.K = K; g.ksplit = 1;
        g.A = dense(space, xoff, xld, 1, 1);
        if (pb) { g.B.kind = OPK_PERMW; g.B.space = SP_PAR; g.B.off = woff; g.B.ld = K; g.B.pb = pb; g.B.pc = pc; g.B.kfast = 1; }
        else g.B = dense(SP_PAR, woff, 1, K, 1);
        g.out.kind = OUT_STORE; g.out.space = SP_WS; g.out.ldc = out.ld; g.out.act = act; g.out.off = out.off;
        g.out.bias_space = SP_PAR; g.out.bias_off = boff;
        // one row per clip (the style / song-info heads): batched plans on the 64x64 tiling run the clips as the rows of ONE
        // GEMM (GemmDesc.clip_rows) — like the folded weight gradients, one descriptor for all clips
        // (a one-clip plan on this tiling marks them too: the flag also pins the summation order, gemm.hip)
        g.clip_rows = (mfma_plan() && rows == 1 && !pb && space == SP_WS) ? 1 : 0;
        op.fwd.push_back(Step{(g.clip_rows && folds_clips()) ? K_GEMM_FOLD : K_GEMM, (int)gemms.host.size(), 1, tiles(rows, N), 1});
        gemms.host.push_back(g);
        // dW | db  =  (dY o act')^T [X | 1]
        GemmDesc w{}; w.M = N; w.A = actgrad(out.off, out.ld, act, true); w.B = dense(space, xoff, xld, 1, 0, K);
        w.out.pb = pb; w.out.pc = pc;
        op.bwd.push_back(wgrad(stage, w, rows, K, woff, boff));
        if (xgrad) {
            if (pb || space != SP_WS) { err = MST_ERR_UNSUPPORTED; }
            GemmDesc a{}; a.M = rows; a.N = K; a.K = N; a.ksplit = 1;
            a.A = actgrad(out.off, out.ld, act, false);
            a.B = dense(SP_PAR, woff, K, 1, 0);
            a.out.kind = OUT_ACCUM; a.out.space = SP_GRAD; a.out.off = xoff; a.out.ldc = xld; a.out.bias_space = -1; a.out.act = ACT_NONE;
            a.clip_rows = (mfma_plan() && rows == 1 && !pb && space == SP_WS) ? 1 : 0;
            op.bwd.push_back(Step{(a.clip_rows && folds_clips()) ? K_GEMM_FOLD : K_GEMM, (int)gemms.host.size(), 1, tiles(rows, K), 1});
            gemms.host.push_back(a);
        }
        ops.push_back(op);
        return out;
    }
    T linear(int stage, const T& x, bool xgrad, const std::string& pre, int N, int act, const char* name = nullptr) {
        return linear(stage, SP_WS, x.off, x.ld, x.rows, x.cols, xgrad, pre + ".weight", pre + ".bias", N, act, nullptr, 0, 0, name);
    }

    // Conv1d(50 -> OC, k=14, s=7, p=4) over the note axis + leaky, as implicit-im2col GEMM (style/model.py:46-53,78-84)
    T conv(int stage) {
        const int P_ = P();
        T x1 = newT(P_, z.OC * NOCT, "pce_conv");
        const int64_t woff = pt.off("pitched_channels_encoder.beats_conv.module.weight");
        const int64_t boff = pt.off("pitched_channels_encoder.beats_conv.module.bias");
        const int K = NF * NPF * CONV_K;
        Op op; op.stage = stage;
        // batched plans on the 64x64 tiling: forward and weight gradient on conv.hip's kernels (window loads instead of per-element
        // im2col index math, 256 x 64 / 64 x 256 tiles); all clips are rows of ONE launch
        if (folds_clips() && z.OC <= 64 && P_ >= 8 && (int64_t)this->K() * P_ * NF * NPN * NPF < ((int64_t)1 << 32)) {
            ConvDesc c{}; c.P = P_; c.clips = this->K(); c.OC = z.OC; c.x1_off = x1.off; c.w_off = woff; c.b_off = boff;
            c.wp_off = tmp((int64_t)NF * 72 * 64);
            const int64_t rows = (int64_t)this->K() * P_ * NOCT;
            int64_t sp = 256;                                 // 3 column tiles x 256 splits = 768 workgroups: three per CU, all co-resident (166 VGPRs)
            int64_t per = ((rows + sp - 1) / sp + 31) / 32 * 32;
            if (per < 256) per = 256;
            c.rows_per_split = per; c.splits = (int)((rows + per - 1) / per);
            c.slab_stride = (int64_t)z.OC * K + z.OC;
            c.slab_off = tmp(c.slab_stride * c.splits);
            const int ci = (int)convs.host.size();
            convs.host.push_back(c);
            op.fwd.push_back(Step{K_CONV_P, ci, 1, 0, 0});
            op.fwd.push_back(Step{K_CONV_F, ci, 1, 0, 0});
            op.bwd.push_back(Step{K_CONV_W, ci, 1, 0, 0});
            weight_slabs(stage, woff, boff, c.slab_off, c.slab_stride, z.OC, K, c.splits, true);
            ops.push_back(op);
            return x1;
        }
        GemmDesc g{}; g.M = P_ * NOCT; g.N = z.OC; g.K = K; g.ksplit = 1;
        g.A.kind = OPK_IM2COL; g.A.space = SP_EXT0; g.A.off = 0; g.A.ones_at = -1; g.A.kfast = 1;
        g.B.kind = OPK_PERMW; g.B.space = SP_PAR; g.B.off = woff; g.B.ld = K; g.B.pb = CONV_K; g.B.pc = NPF; g.B.kfast = 1;
        g.out.kind = OUT_CONV; g.out.space = SP_WS; g.out.off = x1.off; g.out.ldc = z.OC * NOCT;
        g.out.bias_space = SP_PAR; g.out.bias_off = boff;
        op.fwd.push_back(Step{K_GEMM, (int)gemms.host.size(), 1, tiles(g.M, g.N), 1});
        gemms.host.push_back(g);
        GemmDesc w{}; w.M = z.OC;
        w.A.kind = OPK_CONVGRAD; w.A.space = SP_GRAD; w.A.off = x1.off; w.A.space2 = SP_WS; w.A.off2 = x1.off;
        w.A.oc = z.OC; w.A.kfast = 1;
        w.B.kind = OPK_IM2COL; w.B.space = SP_EXT0; w.B.off = 0; w.B.ones_at = K; w.B.kfast = 0;
        w.out.pb = CONV_K; w.out.pc = NPF;
        // the conv body's folded loader wants >= one k-tile of rows per clip
        op.bwd.push_back(wgrad(stage, w, P_ * NOCT, K, woff, boff, P_ * NOCT >= 64));
        ops.push_back(op);
        return x1;
    }

    // LSTM directions that do not depend on each other: their input projections are ordinary linear
    // ops, the recurrences share ONE launch (blockIdx.y = member), and so do the W_hh-gradient GEMMs.
    struct LstmSpec { T x; int B, S, H, reverse; std::string pre; T out; int coloff; };
    void lstm_group(int stage, const std::vector<LstmSpec>& specs) {
        std::vector<T> zxs;
        for (auto& sp : specs) {
            const std::string sfx = sp.reverse ? "_reverse" : "";
            zxs.push_back(linear(stage, SP_WS, sp.x.off, sp.x.ld, sp.x.rows, sp.x.cols, true, sp.pre + ".weight_ih_l0" + sfx,
                                 sp.pre + ".bias_ih_l0" + sfx, 4 * sp.H, ACT_NONE));
        }
        Op op; op.stage = stage;
        const int first = (int)lstms.host.size(), first_hh = (int)gemms.host.size();
        int maxB = 1, maxH = 1, minH = 1 << 30, maxTiles = 1, maxSplit = 1;
        for (size_t i = 0; i < specs.size(); ++i) {
            const LstmSpec& sp = specs[i];
            const int H = sp.H;
            if (!lstm_hidden_supported(H)) err = MST_ERR_UNSUPPORTED;
            const std::string sfx = sp.reverse ? "_reverse" : "";
            const int64_t whh = pt.off(sp.pre + ".weight_hh_l0" + sfx), bhh = pt.off(sp.pre + ".bias_hh_l0" + sfx);
            const int64_t n = (int64_t)sp.B * sp.S;
            LstmDesc l{}; l.B = sp.B; l.S = sp.S; l.H = H; l.reverse = sp.reverse; l.zx_off = zxs[i].off; l.whh_off = whh; l.bhh_off = bhh;
            l.out_off = sp.out.off + sp.coloff; l.out_ld = sp.out.ld;
            l.gates_off = tmp(n * 4 * H); l.c_off = tmp(n * H); l.hprev_off = tmp(n * H); l.tc_off = tmp(n * H);
            l.gout_off = sp.out.off + sp.coloff; l.gzx_off = zxs[i].off;
            l.whht_off = H > 64 ? tmp((int64_t)4 * H * H) : 0;
            // the LSTM_NB workgroups of a sequence wait for each other, so every workgroup of the launch must be resident at once:
            // one group per clip, as many as coresident_slots() allows on the device the plan is created on (a partition has fewer
            // CUs); mst_plan_options.lstm_flavour = 1 always takes one workgroup per sequence
            if (opt.lstm_flavour != 1 && H == LSTM_MH && sp.B == 1 && specs.size() == 1 && LSTM_NB * K() <= coresident_slots())
                l.multi = opt.lstm_flavour == 2 ? 2 : 1;
            l.xch_off = l.multi ? tmp(2 * (2 * H + 2 * 4 * H)) : 0;
            l.status_off = status_off;
            lstms.host.push_back(l);
            if (sp.B > maxB) maxB = sp.B;
            if (H > maxH) maxH = H;
            if (H < minH) minH = H;
            // W_hh | b_hh: the directions' weight-gradient GEMMs share one launch (pushed behind the recurrences)
            GemmDesc w{}; w.M = 4 * H;
            w.A = dense(SP_GRAD, zxs[i].off, 1, 4 * H, 0);
            w.B = dense(SP_TMP, l.hprev_off, H, 1, 0, H);
            const Step ws = wgrad(stage, w, (int)n, H, whh, bhh, true, (int)specs.size());
            maxTiles = std::max(maxTiles, ws.a);
            maxSplit = std::max(maxSplit, ws.b);
        }
        if (lstm_band(maxH) != lstm_band(minH)) err = MST_ERR_UNSUPPORTED;       // one register / L2 / wide flavour per launch
        const int cnt = (int)specs.size();
        if (maxH > 64) op.fwd.push_back(Step{K_LSTM_T, first, cnt, 0, maxH});
        op.fwd.push_back(Step{K_LSTM_F, first, cnt, maxB, maxH});
        op.bwd.push_back(Step{K_LSTM_B, first, cnt, maxB, maxH});
        op.bwd.push_back(Step{folds_clips() ? K_GEMM_FOLD : K_GEMM, first_hh, cnt, maxTiles, maxSplit});
        ops.push_back(op);
    }
    void lstm(int stage, const T& x, int B, int S, int H, int reverse, const std::string& pre, const T& out, int coloff) {
        lstm_group(stage, {LstmSpec{x, B, S, H, reverse, pre, out, coloff}});
    }

    // nn.Linear with K_in <= 8 over a very tall, contiguous input: one lane per row instead of a GEMM of tile padding
    T rowlin(int stage, const T& x, bool xgrad, const std::string& pre, int N, int act, const char* name = nullptr) {
        if (!rowlin_supported(x.cols, N) || x.ld != x.cols) return linear(stage, x, xgrad, pre, N, act, name);
        T out = newT(x.rows, N, name);
        RowLinDesc r{}; r.rows = x.rows; r.kin = x.cols; r.nout = N; r.act = act; r.xgrad = xgrad ? 1 : 0;
        r.x_off = x.off; r.y_off = out.off; r.w_off = pt.off(pre + ".weight"); r.b_off = pt.off(pre + ".bias");
        if (r.b_off != r.w_off + (int64_t)N * x.cols) err = MST_ERR_UNSUPPORTED;
        const int want = (x.rows + 255) / 256;
        const int cap = K() == 1 ? 128 : (1024 / K() < 4 ? 4 : (1024 / K() > 128 ? 128 : 1024 / K()));
        r.nblk = want < cap ? want : cap;
        r.slab_stride = N * x.cols + N; r.slab_off = tmp((int64_t)r.slab_stride * r.nblk);
        Op op; op.stage = stage;
        op.fwd.push_back(Step{K_ROW_F, (int)rowlins.host.size(), 1, 0, 0});
        op.bwd.push_back(Step{K_ROW_B, (int)rowlins.host.size(), 1, 0, 0});
        rowlins.host.push_back(r); ops.push_back(op);
        slabs[stage_idx(stage)].push_back(SlabEntry{r.w_off, r.slab_off, r.slab_stride, r.slab_stride, r.nblk});
        return out;
    }

    // One column block of a Linear whose input is a broadcast-concat (style/utils/pytorch.py:54-65 + nn.Linear):
    //   out[:, col0 : col0 + N] (+)= x (rows x kb) . W[:, k0 : k0 + kb]^T  [+ bias],   no activation.
    // W is the full (N x Kfull) parameter; the bias is the Linear's parameter bias (bname), a one-row activation tensor
    // (bias_act: its gradient is the column sum of dY) or absent.  The concat itself is never formed: the caller adds the
    // blocks' outputs where it consumes them.  Backward: weight-gradient block through a 2-D slab entry, dx += dY . W block.
    // act != ACT_NONE: the block carries the Linear's activation (the weight / input gradients then read dY o act'(Y));
    // row_bias + bias_div: output row m also adds row m / bias_div of `row_bias` (the sum of the Linear's broadcast blocks);
    // its gradient is the sum of dY o act' over each group of bias_div rows.
    void linear_part(int stage, const T& x, bool xgrad, const std::string& wname, int k0, int Kfull, const std::string& bname,
                     const T* bias_act, int N, const T& out, int col0, int act = ACT_NONE, const T* row_bias = nullptr, int bias_div = 0) {
        const int rows = x.rows, kb = x.cols;
        const int64_t woff = pt.off(wname) + k0;
        Op op; op.stage = stage;
        GemmDesc g{}; g.M = rows; g.N = N; g.K = kb; g.ksplit = 1;
        g.A = dense(SP_WS, x.off, x.ld, 1, 1);
        g.B = dense(SP_PAR, woff, 1, Kfull, 1);
        g.out.kind = OUT_STORE; g.out.space = SP_WS; g.out.ldc = out.ld; g.out.act = act; g.out.off = out.off + col0;
        g.out.bias_space = -1;
        if (!bname.empty()) { g.out.bias_space = SP_PAR; g.out.bias_off = pt.off(bname); }
        else if (bias_act) { g.out.bias_space = SP_WS; g.out.bias_off = bias_act->off + col0; }
        else if (row_bias) { g.out.bias_space = SP_WS; g.out.bias_off = row_bias->off; g.out.bias_div = bias_div; g.out.bias_ld = row_bias->ld; }
        if (row_bias && (rows % bias_div || row_bias->rows != rows / bias_div || row_bias->cols != N)) err = MST_ERR_UNSUPPORTED;
        op.fwd.push_back(Step{K_GEMM, (int)gemms.host.size(), 1, tiles(rows, N), 1});
        gemms.host.push_back(g);
        // dW block | db  =  dY^T [X | 1]
        const bool pbias = !bname.empty();
        const int64_t dy = out.off + col0;
        GemmDesc w{}; w.M = N;
        w.A = act != ACT_NONE ? actgrad(dy, out.ld, act, true) : dense(SP_GRAD, dy, 1, out.ld, 0);
        w.B = dense(SP_WS, x.off, x.ld, 1, 0, pbias ? kb : -1);
        op.bwd.push_back(wgrad(stage, w, rows, kb, woff, pbias ? pt.off(bname) : -1, true, 1, Kfull, pt.off(wname)));
        if (xgrad) {
            GemmDesc a{}; a.M = rows; a.N = kb; a.K = N; a.ksplit = 1;
            a.A = act != ACT_NONE ? actgrad(dy, out.ld, act, false) : dense(SP_GRAD, dy, out.ld, 1, 1);
            a.B = dense(SP_PAR, woff, Kfull, 1, 0);
            a.out.kind = OUT_ACCUM; a.out.space = SP_GRAD; a.out.off = x.off; a.out.ldc = x.ld; a.out.bias_space = -1; a.out.act = ACT_NONE;
            op.bwd.push_back(Step{K_GEMM, (int)gemms.host.size(), 1, tiles(rows, kb), 1});
            gemms.host.push_back(a);
        }
        if (bias_act) column_sum(op, dy, out.ld, rows, N, bias_act->off + col0);
        if (row_bias) {          // g_row_bias[j] += sum of (dY o act')[j * bias_div .. + bias_div)
            SegRedDesc r{}; r.src_off = out.off; r.src_ld = out.ld; r.start = col0; r.width = N;
            r.dst_off = row_bias->off; r.dst_ld = row_bias->ld; r.nidx = rows / bias_div;
            const int rs[4] = {rows / bias_div, bias_div, 1, 1};
            for (int q = 0; q < 4; ++q) { r.d[q] = rs[q]; r.s[q] = 0; r.kd[q] = 1; }
            r.s[0] = 1; r.kd[0] = rows / bias_div;
            const int stage2 = partials(r, bias_div);
            r.act = act; r.y_off = out.off;
            op.bwd.push_back(Step{K_SEGRED, (int)segreds.host.size(), 1, r.nidx * r.nchunk, stage2});
            segreds.host.push_back(r);
        }
        ops.push_back(op);
    }

    // nn.Linear + activation over cat_with_broadcast(segments) without the concat: the segment that varies along every
    // row-space dim goes through one GEMM whose epilogue adds, per group of rs[3] rows, the SUM of the other segments' blocks
    // (each a small GEMM over its own rows, added up by a broadcast-sum gather); none of the broadcast copies is ever formed.
    //   out[r] = act( x_full[r] W_full^T + sum_i (x_i W_i^T)[index_i(r)] + b )
    // Requires: exactly one full segment (stride pattern of a dense row index), every other segment constant along dim 3.
    T linear_bcast(int stage, const int rs[4], const std::vector<SegIn>& segs, const std::vector<T>& xs, const std::vector<bool>& xg,
                   const std::string& pre, int N, int act, const char* name = nullptr) {
        const int rows = rs[0] * rs[1] * rs[2] * rs[3], mid = rs[0] * rs[1] * rs[2];
        int Kfull = 0, full = -1;
        for (auto& sg : segs) Kfull += sg.width;
        for (size_t i = 0; i < segs.size(); ++i) if (xs[i].rows == rows) full = (int)i;
        if (full < 0) { err = MST_ERR_UNSUPPORTED; return T{}; }
        const std::string wname = pre + ".weight", bname = pre + ".bias";
        std::vector<SegIn> parts;
        int k0 = 0;
        bool bias_done = false;
        for (size_t i = 0; i < segs.size(); ++i) {
            if ((int)i != full) {
                if (segs[i].s[3] != 0) err = MST_ERR_UNSUPPORTED;
                T P = newT(xs[i].rows, N);
                const bool with_bias = !bias_done && xs[i].rows == 1;      // the parameter bias rides on a one-row block
                linear_part(stage, xs[i], xg[i], wname, k0, Kfull, with_bias ? bname : std::string(), nullptr, N, P, 0);
                bias_done |= with_bias;
                SegIn ps = segs[i]; ps.space = SP_WS; ps.off = P.off; ps.ld = P.ld; ps.width = N; ps.grad = true;
                parts.push_back(ps);
            }
            k0 += segs[i].width;
        }
        if (!bias_done) { err = MST_ERR_UNSUPPORTED; return T{}; }
        const int rsm[4] = {rs[0], rs[1], rs[2], 1};
        T S = gather(stage, rsm, parts, true);
        if (S.rows != mid) err = MST_ERR_UNSUPPORTED;
        T out = newT(rows, N, name);
        k0 = 0;
        for (int i = 0; i < full; ++i) k0 += segs[i].width;
        linear_part(stage, xs[full], xg[full], wname, k0, Kfull, std::string(), nullptr, N, out, 0, act, &S, rs[3]);
        return out;
    }

    // backward helper: g[dst_off .. + width) += sum over `rows` rows of g[src_off + r * src_ld .. + width)
    void column_sum(Op& op, int64_t src_off, int src_ld, int rows, int width, int64_t dst_off) {
        SegRedDesc r{}; r.src_off = src_off; r.src_ld = src_ld; r.start = 0; r.width = width; r.dst_off = dst_off; r.dst_ld = width; r.nidx = 1;
        const int rs[4] = {rows, 1, 1, 1};
        for (int q = 0; q < 4; ++q) { r.d[q] = rs[q]; r.s[q] = 0; r.kd[q] = 1; }
        const int stage2 = partials(r, rows);
        op.bwd.push_back(Step{K_SEGRED, (int)segreds.host.size(), 1, r.nidx * r.nchunk, stage2});
        segreds.host.push_back(r);
    }

    // tiled: the exchange of one workspace range over the ranks (all-reduce SUM, done by the host between two phases).
    // forward = the activation range, backward = the same range of the gradient arena (bwd_too), or a scratch range
    void exchange(Op& op, int space, int64_t off, int len, bool bwd_too) {
        op.fwd.push_back(Step{K_XCHG, (int)xchgs.size(), 1, 0, 0});
        xchgs.push_back(Xchg{space, off, len});
        if (space == SP_WS)          // the other ranks' rows must be zero when the SUM runs
            for (int64_t at = off; at < off + len; at += 16384) zero_fwd.push_back(ZeroChunk{at, (int32_t)std::min<int64_t>(16384, off + len - at), 0});
        if (bwd_too) { op.bwd.insert(op.bwd.begin(), Step{K_XCHG, (int)xchgs.size(), 1, 0, 0}); xchgs.push_back(Xchg{SP_GRAD, off, len}); }
    }
    // tiled: this rank's rows of a per-bar tensor into their place in a buffer that holds every rank's rows (the others'
    // rows are zero, so that the exchange's SUM is an all-gather); backward: gather the owned rows' gradient back
    void copy_rows(Op& op, int64_t src_off, int src_sa, int src_sb, int64_t dst_off, int dst_sa, int dst_sb, int na, int nb, int cols) {
        CopyDesc c{}; c.src_off = src_off; c.dst_off = dst_off; c.na = na; c.nb = nb; c.cols = cols;
        c.src_sa = src_sa; c.src_sb = src_sb; c.dst_sa = dst_sa; c.dst_sb = dst_sb;
        op.fwd.insert(op.fwd.begin(), Step{K_COPY_F, (int)copies.host.size(), 1, 0, 0});
        op.bwd.push_back(Step{K_COPY_B, (int)copies.host.size(), 1, 0, 0});
        copies.host.push_back(c);
    }
    // tiled: rank-local partial sums -> `sum` (exchanged) -> back as the only non-zero partial
    void fold_exchange(std::vector<Step>& steps, size_t at, int space, int64_t part_off, int nrows, int row_stride, int ncols,
                       int col_stride) {
        FoldDesc f{}; f.space = space; f.part_off = part_off; f.nrows = nrows; f.row_stride = row_stride; f.ncols = ncols;
        f.col_stride = col_stride; f.sum_off = tmp(ncols);
        const int fi = (int)folds.host.size();
        folds.host.push_back(f);
        const int xi = (int)xchgs.size();
        xchgs.push_back(Xchg{SP_TMP, f.sum_off, ncols});
        std::vector<Step> ins = {Step{K_FOLD, fi, 1, 0, 0}, Step{K_XCHG, xi, 1, 0, 0}, Step{K_SPREAD, fi, 1, 0, 0}};
        steps.insert(steps.begin() + at, ins.begin(), ins.end());
    }

    // global = true (tiled plans): the slices hold this rank's rows only, the norms are over every rank's rows
    void combine(int stage, int64_t x_off, int rows, int cols, int ld, int64_t cs, int Cn, const T& out, bool global = false) {
        CombineDesc c{}; c.Cn = Cn; c.rows = rows; c.cols = cols; c.ld = ld; c.x_off = x_off; c.cs = cs; c.out_off = out.off;
        c.stats_off = tmp(64); c.part_off = tmp(COMBINE_MAXBLK * (COMBINE_MAXC + 1));
        c.gx_off = x_off; c.gout_off = out.off;
        if ((int64_t)rows * cols >= ((int64_t)1 << 31)) err = MST_ERR_UNSUPPORTED;      // the kernels index a slice with 32 bits
        int64_t nb = ((int64_t)rows * cols + 1023) / 1024;
        c.nblk = (int)(nb < 1 ? 1 : (nb > COMBINE_MAXBLK ? COMBINE_MAXBLK : nb));
        const int large = (int64_t)rows * cols > COMBINE_SMALL ? 1 : 0;     // Step.b: 1 = needs the two-launch path
        Op op; op.stage = stage;
        if (global && tiled()) {
            const int ci = (int)combines.host.size();
            op.fwd = {Step{K_COMB_F1, ci, 1, c.nblk, 0}, Step{K_COMB_F2, ci, 1, c.nblk, 0}};
            fold_exchange(op.fwd, 1, SP_TMP, c.part_off, c.nblk, COMBINE_MAXC + 1, Cn, 1);
            op.bwd = {Step{K_COMB_B1, ci, 1, c.nblk, 0}, Step{K_COMB_B2, ci, 1, c.nblk, 0}};
            fold_exchange(op.bwd, 1, SP_TMP, c.part_off, c.nblk, COMBINE_MAXC + 1, Cn + 1, 1);
        } else {
            op.fwd.push_back(Step{K_COMB_F, (int)combines.host.size(), 1, c.nblk, large});
            op.bwd.push_back(Step{K_COMB_B, (int)combines.host.size(), 1, c.nblk, large});
        }
        combines.host.push_back(c);
        ops.push_back(op);
    }

    void build();
    void accesses(const Step& s, std::vector<Acc>& out, bool scheduled = false) const;
    void first_writers(std::vector<Step>& list, size_t begin, bool per_stage, std::vector<Acc>& zero);
    void schedule_pass(const std::vector<Step>& seq, std::vector<Step>& out, bool across_stages);
    int ride_slot(const Step& s) const;
    bool assign_streams(std::vector<Step>& L);
    int n_signals = 0;                 // event slots assign_streams handed out (<= N_EVENTS)
    void schedule();
    int upload();
};

static const int RS1[4] = {1, 1, 1, 1};

void mst_plan::build() {
    // R = the bars this plan computes per-position work for (its tile when tiled), Rt = the clip's bars: the bar-level chains
    // (bars LSTMs, style encoder, song-info bars LSTM) run replicated over all Rt bars on every rank
    const int C = d.C, R = Rl(), Rt = d.R, r0 = tiled() ? opt.tile_r0 : 0, Tn = d.T, P_ = P(), Q_ = Q();
    const bool TL = tiled();
    const bool U = d.has_unpitched != 0;
    const int E = MST_STAGE_EXTRACT, IN = MST_STAGE_INFO, AP = MST_STAGE_APPLY;
    // ---- inputs / targets (never zeroed, written by the host side)
    T instr = newT(C, z.I, "instr"), mode = newT(1, 2, "mode"), bpm = newT(1, 1, "bpm");
    newT(1, z.NI, "used_instruments"); newT(1, 1, "bpm_target");
    status_off = newT(1, 64, "device_status").off;       // int32 word 0: MST_DEV_* bits (activation arena: never part of a zero list)
    t_losses = newT(1, 64, "losses"); t_saved = newT(1, MST_LOSS_SAVED, "loss_saved"); t_gl = newT(1, 64, "grad_losses");
    loss_scratch = tmp(mst_loss_scratch_floats());
    auto seg0 = [&](const T& t) { return seg(t, 0, 0, 0, 0, true); };      // broadcast over every row

    // ================================================================= stage 1: extract_style
    std::string m = "pitched_channels_encoder";
    T pce_il = linear(E, instr, false, m + ".instruments_linear", z.PCE_IL, ACT_LEAKY);
    T x1 = conv(E);
    const int rsCQ[4] = {C, R * Tn, 1, 1};
    T pcat = gather(E, rsCQ, {seg(x1, R * Tn, 1, 0, 0), seg(pce_il, 1, 0, 0, 0)});
    T pa = linear(E, pcat, true, m + ".linear", z.H, ACT_LEAKY);
    const std::string mu = "unpitched_channels_encoder";
    T pbeats = newT(P_, z.H, "pitched_beats"), ubeats{}, ua{};
    std::vector<LstmSpec> beat_group = {LstmSpec{pa, C * R, Tn, z.H, 0, m + ".beats_lstm.module", pbeats, 0}};
    if (U) {
        ua = linear(E, SP_EXT1, 0, NF * NUN * NUF, Q_, NF * NUN * NUF, false, mu + ".linear.weight", mu + ".linear.bias",
                    z.H, ACT_LEAKY, nullptr, NUN, NUF);
        ubeats = newT(Q_, z.H, "unpitched_beats");
        beat_group.push_back(LstmSpec{ua, R, Tn, z.H, 0, mu + ".beats_lstm.module", ubeats, 0});
    }
    lstm_group(E, beat_group);
    T plast = newT(Rt, z.H), ulast{};
    T pbl_all{}, ubl_all{};
    if (TL) {
        // last-beat states of every rank's bars, bar-major [(bar, channel), H] | [bar, H]: own rows copied in, one exchange
        pbl_all = newT(Rt * C, z.H);
        if (U) ubl_all = newT(Rt, z.H);
        Op op; op.stage = E;
        exchange(op, SP_WS, pbl_all.off, (int)((U ? ubl_all.off + (int64_t)Rt * z.H : pbl_all.off + (int64_t)Rt * C * z.H) - pbl_all.off), true);
        copy_rows(op, pbeats.off + (int64_t)(Tn - 1) * z.H, Tn * z.H, R * Tn * z.H, pbl_all.off + (int64_t)r0 * C * z.H, C * z.H, z.H, R, C, z.H);
        if (U) copy_rows(op, ubeats.off + (int64_t)(Tn - 1) * z.H, Tn * z.H, 0, ubl_all.off + (int64_t)r0 * z.H, z.H, 0, R, 1, z.H);
        ops.push_back(op);
        combine(E, pbl_all.off, Rt, z.H, C * z.H, z.H, C, plast);
    } else
        combine(E, pbeats.off + (int64_t)(Tn - 1) * z.H, R, z.H, Tn * z.H, (int64_t)R * Tn * z.H, C, plast);
    T pbars = newT(Rt, 2 * z.HB, "pitched_bars"), ubars{};
    std::vector<LstmSpec> bar_group = {LstmSpec{plast, 1, Rt, z.HB, 0, m + ".bars_lstm", pbars, 0},
                                       LstmSpec{plast, 1, Rt, z.HB, 1, m + ".bars_lstm", pbars, z.HB}};
    if (U) {
        ulast = newT(Rt, z.H);
        if (TL) combine(E, ubl_all.off, Rt, z.H, z.H, 0, 1, ulast);
        else combine(E, ubeats.off + (int64_t)(Tn - 1) * z.H, R, z.H, Tn * z.H, 0, 1, ulast);
        ubars = newT(Rt, 2 * z.HB, "unpitched_bars");
        bar_group.push_back(LstmSpec{ulast, 1, Rt, z.HB, 0, mu + ".bars_lstm", ubars, 0});
        bar_group.push_back(LstmSpec{ulast, 1, Rt, z.HB, 1, mu + ".bars_lstm", ubars, z.HB});
    }
    lstm_group(E, bar_group);
    // this rank's bars of the (replicated) bar tensors
    const T pbars_own{pbars.off + (int64_t)r0 * pbars.ld, R, pbars.cols, pbars.ld};
    const T ubars_own = U ? T{ubars.off + (int64_t)r0 * ubars.ld, R, ubars.cols, ubars.ld} : T{};

    m = "pitched_rhythm_encoder";
    T pre_il = linear(E, instr, false, m + ".instruments_linear", z.PRE_IL, ACT_LEAKY);
    T pre_ml = linear(E, mode, false, m + ".mode_linear", z.PRE_ML, ACT_LEAKY);
    T pre_bp = linear(E, bpm, false, m + ".bpm_linear", z.PRE_BPL, ACT_LEAKY);
    T pre_bl = linear(E, pbeats, true, m + ".beats_linear", z.PRE_BL, ACT_LEAKY);
    T pre_br = linear(E, pbars_own, true, m + ".bars_linear", z.PRE_BRL, ACT_LEAKY);
    T pre_cl = linear(E, SP_EXT0, 0, NPN * NPF, P_ * NF, NPN * NPF, false, m + ".channels_linear.weight",
                      m + ".channels_linear.bias", z.PRE_CL, ACT_LEAKY);
    const int rsCRTF[4] = {C, R, Tn, NF};
    // Linear over cat_with_broadcast(beats, bars, channels, instruments, mode, bpm) (style/model.py rhythm encoders) with the
    // concat decomposed away: only the per-fraction `channels` block runs at full row count
    T prh_c = linear_bcast(E, rsCRTF,
                           {seg(pre_bl, R * Tn, Tn, 1, 0), seg(pre_br, 0, 1, 0, 0), seg(pre_cl, R * Tn * NF, Tn * NF, NF, 1),
                            seg(pre_il, 1, 0, 0, 0), seg0(pre_ml), seg0(pre_bp)},
                           {pre_bl, pre_br, pre_cl, pre_il, pre_ml, pre_bp}, {true, true, true, true, true, true},
                           m + ".linear", z.RH, ACT_LEAKY);
    T prh = newT(Q_ * NF, z.RH, "pitched_rhythm");
    combine(E, prh_c.off, Q_ * NF, z.RH, z.RH, (int64_t)Q_ * NF * z.RH, C, prh, true);

    T bars = pbars, rhythm = prh;
    if (U) {
        m = "unpitched_rhythm_encoder";
        T ure_bp = linear(E, bpm, false, m + ".bpm_linear", z.PRE_BPL, ACT_LEAKY);
        T ure_bl = linear(E, ubeats, true, m + ".beats_linear", z.PRE_BL, ACT_LEAKY);
        T ure_br = linear(E, ubars_own, true, m + ".bars_linear", z.PRE_BRL, ACT_LEAKY);
        T ure_cl = linear(E, SP_EXT1, 0, NUN * NUF, Q_ * NF, NUN * NUF, false, m + ".channels_linear.weight",
                          m + ".channels_linear.bias", z.URE_CL, ACT_LEAKY);
        const int rs1RTF[4] = {1, R, Tn, NF};
        T urh_c = linear_bcast(E, rs1RTF, {seg(ure_bl, 0, Tn, 1, 0), seg(ure_br, 0, 1, 0, 0), seg(ure_cl, 0, Tn * NF, NF, 1), seg0(ure_bp)},
                               {ure_bl, ure_br, ure_cl, ure_bp}, {true, true, true, true}, m + ".linear", z.RH, ACT_LEAKY);
        T urh = newT(Q_ * NF, z.RH, "unpitched_rhythm");
        combine(E, urh_c.off, Q_ * NF, z.RH, z.RH, 0, 1, urh, true);
        // combine(pitched, unpitched) stacks the pair on a new leading axis (style/model.py:766-767)
        bars = newT(Rt, z.BAR, "bars");
        combine(E, pbars.off, Rt, z.BAR, z.BAR, ubars.off - pbars.off, 2, bars);
        rhythm = newT(Q_ * NF, z.RH, "rhythm");
        combine(E, prh.off, Q_ * NF, z.RH, z.RH, urh.off - prh.off, 2, rhythm, true);
    } else {
        named["bars"] = bars; named["rhythm"] = rhythm;
    }

    m = "style_encoder";
    T se_il = linear(E, instr, false, m + ".instruments_linear", z.SE_IL, ACT_LEAKY);
    T se_ml = linear(E, mode, false, m + ".mode_linear", z.SE_ML, ACT_LEAKY);
    T se_bp = linear(E, bpm, false, m + ".bpm_linear", z.SE_BL, ACT_LEAKY);
    T sel = newT(Rt, z.SE_L);
    lstm(E, bars, 1, Rt, z.SE_L, 0, m + ".bars_lstm", sel, 0);
    T sel_last{sel.off + (int64_t)(Rt - 1) * z.SE_L, 1, z.SE_L, z.SE_L};
    const int rsC[4] = {C, 1, 1, 1};
    T secat = gather(E, rsC, {seg0(sel_last), seg(se_il, 1, 0, 0, 0), seg0(se_ml), seg0(se_bp)});
    T se_lin = linear(E, secat, true, m + ".linear", z.STYLE, ACT_LEAKY);
    T style = newT(1, z.STYLE, "style");
    combine(E, se_lin.off, 1, z.STYLE, z.STYLE, z.STYLE, C, style);

    m = "melody_encoder";
    T me_il = linear(E, instr, false, m + ".instruments_linear", z.ME_IL, ACT_LEAKY);
    T me_bl = linear(E, pbeats, true, m + ".beats_linear", z.ME_BL, ACT_LEAKY);
    T me_br = linear(E, pbars_own, true, m + ".bars_linear", z.ME_BRL, ACT_LEAKY);
    const int rsCRT[4] = {C, R, Tn, 1};
    T ycat = gather(E, rsCRT, {seg(me_bl, R * Tn, Tn, 1, 0), seg(me_br, 0, 1, 0, 0), seg(me_il, 1, 0, 0, 0)});
    T me_oct = linear(E, ycat, true, m + ".octave_linear", z.MEL * NOCT, ACT_LEAKY);
    T me_deg = linear(E, ycat, true, m + ".scale_degree_linear", z.MEL * NDEG, ACT_LEAKY);
    // note tail + channel combine fused (notes.hip): melody is written directly, the per-channel tensor never exists
    T melody = newT(Q_ * NF * NPN, z.MEL, "melody");
    {
        NotesDesc n{}; n.C = C; n.Q = Q_; n.W = z.MEL; n.CW = z.ME_CW; n.ML = z.PSA_ML;
        n.oct_off = me_oct.off; n.deg_off = me_deg.off; n.x_off = 0; n.x_space = SP_EXT0;
        n.wc_off = pt.off(m + ".channels_linear.weight"); n.bc_off = pt.off(m + ".channels_linear.bias");
        n.wl_off = pt.off(m + ".linear.weight"); n.bl_off = pt.off(m + ".linear.bias");
        n.out_off = melody.off; n.g_out_off = melody.off; n.g_oct_off = me_oct.off; n.g_deg_off = me_deg.off;
        const int nw = z.ME_CW * NPF + z.ME_CW + z.MEL * (z.MEL + z.ME_CW) + z.MEL;
        // reduction passes: waves per channel (one partial each), a wave per position up to 64
        // (the same count for every clip count: the grouping of the partial sums decides the last bits of n_c, and a clip's
        // activations are bit-identical in one-clip and batched plans)
        n.nwc = Q_ < 64 ? Q_ : 64;
        // forward: a wave per (q, group of fractions).  One clip per launch is latency-bound and wants every wave it can get
        // (a wave per fraction: 10 x Q waves); batched plans have the clips for that and keep two waves per q
        n.fhn = K() == 1 ? NF : 2;
        n.part_off = tmp((int64_t)(C + 1) * n.nwc); n.stats_off = tmp(C + 1);
        // backward: two waves per position (one per half of the fractions), two positions per workgroup up to the cap; every
        // wave leaves one slab row for the deferred reduction
        const int me_blk = K() == 1 ? 256 : (2048 / K() < 4 ? 4 : (2048 / K() > 256 ? 256 : 2048 / K()));
        const int want = (P_ + 1) / 2;
        n.nblk = want < me_blk ? want : me_blk; n.slab_stride = nw; n.slab_off = tmp((int64_t)nw * n.nblk);
        Op op; op.stage = E;
        const int ni = (int)notes.host.size();
        op.fwd.push_back(Step{K_ME_SQ, ni, 1, 0, 0});
        op.fwd.push_back(Step{K_ME_F, ni, 1, 0, 0});
        op.bwd.push_back(Step{K_ME_RED, ni, 1, 0, 0});
        op.bwd.push_back(Step{K_ME_B, ni, 1, 0, 0});
        if (TL) {      // the channel norms are over every rank's positions
            fold_exchange(op.fwd, 1, SP_TMP, n.part_off, n.nwc, 1, C, n.nwc);
            fold_exchange(op.bwd, 1, SP_TMP, n.part_off, n.nwc, 1, C + 1, n.nwc);
        }
        notes.host.push_back(n); ops.push_back(op);
        // channels_linear.{weight,bias}, linear.{weight,bias} are contiguous in the flat buffer
        slabs[0].push_back(SlabEntry{n.wc_off, n.slab_off, nw, nw, n.nblk});
    }

    // ================================================================= stage 2: predict_song_info
    m = "song_info_model";
    T rhy_rows{rhythm.off, Q_, NF * z.RH, NF * z.RH};                    // squash_dims(rhythm, -2)
    T sbl = newT(Q_, z.SIM_BL);
    lstm(IN, rhy_rows, R, Tn, z.SIM_BL, 0, m + ".beats_lstm.module", sbl, 0);
    T slast{sbl.off + (int64_t)(Tn - 1) * z.SIM_BL, R, z.SIM_BL, Tn * z.SIM_BL};
    if (TL) {          // every rank's last-beat rhythm features, then the bars LSTM replicated
        T sl_all = newT(Rt, z.SIM_BL);
        Op op; op.stage = IN;
        exchange(op, SP_WS, sl_all.off, Rt * z.SIM_BL, true);
        copy_rows(op, slast.off, Tn * z.SIM_BL, 0, sl_all.off + (int64_t)r0 * z.SIM_BL, z.SIM_BL, 0, R, 1, z.SIM_BL);
        ops.push_back(op);
        slast = sl_all;
    }
    T sbr = newT(Rt, z.NRF);
    lstm(IN, slast, 1, Rt, z.NRF, 0, m + ".bars_lstm", sbr, 0);
    T feats{sbr.off + (int64_t)(Rt - 1) * z.NRF, 1, z.NRF, z.NRF};
    struct Head { const char* nm; int sw, rw, n, act; const char* out; };
    const Head heads[3] = {{"instruments", z.SIM_SI, z.SIM_RI, z.NI, ACT_NONE, "instruments_pred"},
                           {"mode", z.SIM_SM, z.SIM_RM, 2, ACT_NONE, "mode_pred"},
                           {"bpm", z.SIM_SB, z.SIM_RB, 1, ACT_BPM, "bpm_pred"}};
    for (const Head& h : heads) {
        T hs = linear(IN, style, true, m + ".style_" + h.nm + "_linear", h.sw, ACT_LEAKY);
        T hr = linear(IN, feats, true, m + ".rhythm_" + h.nm + "_linear", h.rw, ACT_LEAKY);
        T hcat = gather(IN, RS1, {seg0(hs), seg0(hr)});
        linear(IN, hcat, true, m + "." + h.nm + "_linear", h.n, h.act, h.out);
    }

    // ================================================================= stage 3: apply_style
    m = "pitched_style_applier";
    T psa_sl = linear(AP, style, true, m + ".style_linear", z.PSA_SL, ACT_LEAKY);
    T psa_rl = linear(AP, rhythm, true, m + ".rhythm_linear", z.PSA_RL, ACT_LEAKY);
    T psa_il = linear(AP, instr, false, m + ".instruments_linear", z.PSA_IL, ACT_LEAKY);
    // octave_linear / scale_degree_linear (88 -> 240 / 210) act on cat_with_broadcast([style (1), rhythm (q, f), instrument (c)]):
    // per row that is 39 600 multiply-adds of which all but the rhythm block repeat for every row.  The pre-activations
    // decompose exactly into z[c, qf] = rt[qf] + it[c] (it = instrument block + style block + bias), three small column-block
    // GEMMs each (linear_part); the note kernels add and activate on the fly, and the (positions x 450) octave / degree tensors
    // and the (positions x 88) concat are never written.  The backward note kernel leaves dL/dz per row; its column sums over c
    // and over qf are the gradients of rt and it.
    const int KA = z.PSA_SL + z.PSA_RL + z.PSA_IL, QF_ = Q_ * NF;
    // backward note kernel: one workgroup per qf (a wave per channel pair) up to a cap sized to keep ~15 waves per CU busy over
    // all clips; every workgroup leaves one row of weight-gradient partials and one row of it-gradient partials
    const int psa_np = psa_bwd_waves(C);
    int psa_nblk;
    {
        const int cap = K() == 1 ? 320 : std::max(4, (256 * 15) / (K() * psa_np));
        psa_nblk = std::min(QF_, cap);
    }
    T rt_x[2], it_x[2], itp_x[2];
    for (int which = 0; which < 2; ++which) {
        const std::string lin = m + (which ? ".scale_degree_linear" : ".octave_linear");
        const int Nw = NPF * 6 * (which ? NDEG : NOCT);
        T sb = newT(1, Nw);
        it_x[which] = newT(C, Nw); rt_x[which] = newT(QF_, Nw);
        linear_part(AP, psa_sl, true, lin + ".weight", 0, KA, lin + ".bias", nullptr, Nw, sb, 0);
        linear_part(AP, psa_il, true, lin + ".weight", z.PSA_SL + z.PSA_RL, KA, "", &sb, Nw, it_x[which], 0);
        linear_part(AP, psa_rl, true, lin + ".weight", z.PSA_SL, KA, "", nullptr, Nw, rt_x[which], 0);
        // gradient of it[c] = sum over qf of dL/dz[c, qf]: the note kernel sums its own qf's, this sums the workgroups' rows
        // (only the gradient slot of itp is used)
        itp_x[which] = newT(psa_nblk, C * Nw);
        Op op; op.stage = AP;
        column_sum(op, itp_x[which].off, C * Nw, psa_nblk, C * Nw, it_x[which].off);
        ops.push_back(op);
    }
    // melody_linear (W -> ML, leaky; style/model.py:606-610,660-662) has no op of its own: the note kernels apply it per note
    T xp = newT(P_ * NF * NPN, NPF, "pitched_pred");
    {
        NotesDesc n{}; n.C = C; n.Q = Q_; n.W = z.MEL; n.CW = z.ME_CW; n.ML = z.PSA_ML;
        n.rt_oct_off = rt_x[0].off; n.rt_deg_off = rt_x[1].off; n.it_oct_off = it_x[0].off; n.it_deg_off = it_x[1].off;
        n.mel_off = melody.off; n.g_mel_off = melody.off; n.wm_off = pt.off(m + ".melody_linear.weight");
        n.wl_off = pt.off(m + ".linear.weight"); n.bl_off = pt.off(m + ".linear.bias");
        if (pt.off(m + ".melody_linear.bias") != n.wm_off + (int64_t)z.PSA_ML * z.MEL || n.wl_off != n.wm_off + (int64_t)z.PSA_ML * z.MEL + z.PSA_ML ||
            n.bl_off != n.wl_off + (int64_t)NPF * (NPF * 6 + z.PSA_ML))
            err = MST_ERR_UNSUPPORTED;                        // the slab row below is these four parameters back to back
        n.out_off = xp.off; n.g_out_off = xp.off;
        n.itp_oct_off = itp_x[0].off; n.itp_deg_off = itp_x[1].off;
        n.x_space = SP_EXT0; n.x_off = 0;                     // the target of the fused loss backward: the pitched input itself
        n.loss_saved_off = t_saved.off; n.loss_gl_off = t_gl.off;
        const int nw = z.PSA_ML * z.MEL + z.PSA_ML + NPF * (NPF * 6 + z.PSA_ML) + NPF;
        n.nblk = psa_nblk; n.slab_stride = nw; n.slab_off = tmp((int64_t)nw * n.nblk);
        Op op; op.stage = AP;
        op.fwd.push_back(Step{K_PSA_F, (int)notes.host.size(), 1, 0, 0});
        op.bwd.push_back(Step{K_PSA_B, (int)notes.host.size(), 1, 0, 0});
        notes.host.push_back(n); ops.push_back(op);
        slabs[2].push_back(SlabEntry{n.wm_off, n.slab_off, nw, nw, n.nblk});
    }
    if (U) {
        m = "unpitched_style_applier";
        T usa_sl = linear(AP, style, true, m + ".style_linear", NF * z.USA_SL, ACT_LEAKY);
        T usa_rl = linear(AP, rhythm, true, m + ".rhythm_linear", z.USA_RL, ACT_LEAKY);
        T sl_view{usa_sl.off, NF, z.USA_SL, z.USA_SL};                   // x.view(1, 1, 1, n_beat_fractions, -1)
        const int rsQ_F[4] = {Q_, NF, 1, 1};
        T ucat = gather(AP, rsQ_F, {seg(sl_view, 0, 1, 0, 0), seg(usa_rl, NF, 1, 0, 0)});
        T v = linear(AP, ucat, true, m + ".notes_linear", NUN * NUF * 4, ACT_LEAKY);
        T v_rows{v.off, Q_ * NF * NUN, NUF * 4, NUF * 4};                  // x.view(..., n_unpitched_notes, -1)
        rowlin(AP, v_rows, true, m + ".linear", NUF, ACT_SIGOUT, "unpitched_pred");
    }
    if (!widths_supported(z)) err = MST_ERR_UNSUPPORTED;
}

// ------------------------------------------------------------------------------------------ scheduler
// Every launch step's read / write ranges are derived from its descriptors; a step's level is one
// more than the deepest earlier step it conflicts with (RAW / WAR / WAW on overlapping ranges of the
// activation, gradient or scratch arena; parameters and the borrowed note tensors are read-only).
// All steps of one level, stage and kernel are then merged into one launch (blockIdx.y = member).
static void acc_add(std::vector<Acc>& v, int space, int64_t lo, int64_t len, bool w, bool accum = false, bool dense = true) {
    if (space != SP_WS && space != SP_GRAD && space != SP_TMP) return;
    if (len <= 0) return;
    Acc a{space, lo, lo + len, w}; a.accum = accum; a.dense = dense;
    v.push_back(a);
}

static void operand_acc(std::vector<Acc>& v, const Operand& o, int di, int dj, int ones) {
    switch (o.kind) {
    case OPK_DENSE: {
        const int64_t si = o.si < 0 ? -o.si : o.si, sj = o.sj < 0 ? -o.sj : o.sj;
        const int dj_eff = ones >= 0 ? dj - 1 : dj;
        acc_add(v, o.space, o.off, (int64_t)(di - 1) * si + (int64_t)(dj_eff > 0 ? dj_eff - 1 : 0) * sj + 1, false);
        break;
    }
    case OPK_ACTGRAD: {
        const int rows = o.transposed ? dj : di;
        acc_add(v, o.space, o.off, (int64_t)rows * o.ld, false);
        acc_add(v, o.space2, o.off2, (int64_t)rows * o.ld, false);
        break;
    }
    case OPK_CONVGRAD: {
        const int64_t n = (int64_t)(dj / NOCT) * o.oc * NOCT;
        acc_add(v, o.space, o.off, n, false);
        acc_add(v, o.space2, o.off2, n, false);
        break;
    }
    default: break;      // IM2COL / PERMW read the borrowed inputs / parameters
    }
}

void mst_plan::accesses(const Step& s, std::vector<Acc>& v, bool scheduled) const {
    // scheduled: s is a step of a scheduled list, so s.first of a replicated kind indexes the scheduled (per-clip relocated)
    // descriptors; clip 0's copies equal the originals
    const bool sc = scheduled && KINDS[s.kind].sched;
    auto tab = [sc](const auto& t) -> const auto& { return sc ? t.sched : t.host; };
    for (int i = 0; i < s.count; ++i) {
        switch (s.kind) {
        case K_GEMM: case K_GEMM_FOLD: {
            const GemmDesc& g = tab(gemms)[s.first + i];
            const int gk = g.fold_rows ? g.fold_rows : g.K;      // a folded reduction touches, per clip, what one clip's would
            const int gm = g.clip_rows ? 1 : g.M;                // ... and so do clips-as-rows (its scheduled copy has M = clips)
            Operand ga = g.A;
            if (g.clip_rows && ga.kind == OPK_ACTGRAD) ga.ld = gk;       // one row of gk columns (its scheduled pitch is the clip stride)
            operand_acc(v, ga, gm, gk, -1);
            operand_acc(v, g.B, gk, g.N, g.B.ones_at);
            const OutSpec& o = g.out;
            if (o.bias_space >= 0)       // a bias row that is an activation (linear_part); bias_div: one row per bias_div output rows
                acc_add(v, o.bias_space, o.bias_off, o.bias_div > 0 ? (int64_t)((g.M - 1) / o.bias_div) * o.bias_ld + g.N : g.N, false);
            if (o.kind == OUT_STORE) acc_add(v, o.space, o.off, (int64_t)(gm - 1) * o.ldc + g.N, true);
            else if (o.kind == OUT_ACCUM) acc_add(v, o.space, o.off, (int64_t)(gm - 1) * o.ldc + g.N, true, true, g.N == o.ldc || gm == 1);
            else if (o.kind == OUT_CONV) acc_add(v, o.space, o.off, (int64_t)(g.M / NOCT) * o.ldc, true);
            else acc_add(v, o.space, o.off, o.slab_stride * g.ksplit, true);
            break;
        }
        case K_LIN_F: case K_LIN_A: case K_LIN_W: {
            if (i > 0) break;
            const LinDesc& l = lins.host[s.first];
            const int64_t nx = (int64_t)(l.rows - 1) * l.x_ld + l.K, ny = (int64_t)(l.rows - 1) * l.y_ld + l.N;
            if (s.kind == K_LIN_F) { acc_add(v, l.x_space, l.x_off, nx, false); acc_add(v, SP_WS, l.y_off, ny, true); }
            else if (s.kind == K_LIN_W) {
                acc_add(v, l.x_space, l.x_off, nx, false); acc_add(v, SP_WS, l.y_off, ny, false); acc_add(v, SP_GRAD, l.y_off, ny, false);
                acc_add(v, SP_TMP, l.slab_off, l.slab_stride * l.splits, true);
            } else {
                acc_add(v, SP_WS, l.y_off, ny, false); acc_add(v, SP_GRAD, l.y_off, ny, false);
                acc_add(v, SP_GRAD, l.x_off, nx, true, true, l.x_ld == l.K || l.rows == 1);
            }
            break;
        }
        case K_CONV_P: case K_CONV_F: case K_CONV_W: {
            if (i > 0) break;
            const ConvDesc& c = convs.host[s.first];
            const int64_t n = (int64_t)c.P * c.OC * NOCT;
            if (s.kind == K_CONV_P) acc_add(v, SP_TMP, c.wp_off, (int64_t)NF * 72 * 64, true);
            else if (s.kind == K_CONV_F) { acc_add(v, SP_TMP, c.wp_off, (int64_t)NF * 72 * 64, false); acc_add(v, SP_WS, c.x1_off, n, true); }
            else { acc_add(v, SP_WS, c.x1_off, n, false); acc_add(v, SP_GRAD, c.x1_off, n, false); acc_add(v, SP_TMP, c.slab_off, c.slab_stride * c.splits, true); }
            break;
        }
        case K_GATHER: {
            const GatherDesc& g = tab(gathers)[s.first + i];
            for (int q = 0; q < g.nseg; ++q) {
                const Seg& sg = g.seg[q];
                int64_t maxrow = 0;
                for (int k = 0; k < 4; ++k) maxrow += (int64_t)(g.d[k] - 1) * sg.s[k];
                acc_add(v, sg.space, sg.off, maxrow * sg.ld + sg.width, false);
            }
            acc_add(v, SP_WS, g.out_off, (int64_t)g.rows * g.K, true);
            break;
        }
        case K_SEGRED: {
            const SegRedDesc& r = tab(segreds)[s.first + i];
            const int64_t rows = (int64_t)r.d[0] * r.d[1] * r.d[2] * r.d[3];
            acc_add(v, SP_GRAD, r.src_off, rows * r.src_ld, false);
            if (r.act != ACT_NONE) acc_add(v, SP_WS, r.y_off, rows * r.src_ld, false);
            acc_add(v, SP_GRAD, r.dst_off, (int64_t)(r.nidx - 1) * r.dst_ld + r.width, true, true, r.width == r.dst_ld || r.nidx == 1);
            if (r.nchunk > 1) acc_add(v, SP_TMP, r.part_off, (int64_t)r.nidx * r.nchunk * r.width, true);
            break;
        }
        case K_LSTM_T: {
            const LstmDesc& l = tab(lstms)[s.first + i];
            if (l.multi) { acc_add(v, SP_TMP, l.xch_off, 2 * (2 * l.H + 8 * l.H), true); break; }
            if (l.H > 64) acc_add(v, SP_TMP, l.whht_off, (int64_t)4 * l.H * l.H, true);
            break;
        }
        case K_LSTM_F: {
            const LstmDesc& l = tab(lstms)[s.first + i];
            const int64_t n = (int64_t)l.B * l.S;
            acc_add(v, SP_WS, l.zx_off, n * 4 * l.H, false);
            acc_add(v, SP_WS, l.out_off, (n - 1) * l.out_ld + l.H, true);
            acc_add(v, SP_TMP, l.gates_off, n * 4 * l.H, true);
            acc_add(v, SP_TMP, l.c_off, n * l.H, true);
            acc_add(v, SP_TMP, l.hprev_off, n * l.H, true);
            acc_add(v, SP_TMP, l.tc_off, n * l.H, true);
            if (l.multi) acc_add(v, SP_TMP, l.xch_off, 2 * (2 * l.H + 8 * l.H), true);
            else if (l.H > 64) acc_add(v, SP_TMP, l.whht_off, (int64_t)4 * l.H * l.H, false);
            break;
        }
        case K_LSTM_B: {
            const LstmDesc& l = tab(lstms)[s.first + i];
            const int64_t n = (int64_t)l.B * l.S;
            acc_add(v, SP_TMP, l.gates_off, n * 4 * l.H, false);
            acc_add(v, SP_TMP, l.c_off, n * l.H, false);
            acc_add(v, SP_TMP, l.tc_off, n * l.H, false);
            acc_add(v, SP_GRAD, l.gout_off, (n - 1) * l.out_ld + l.H, false);
            acc_add(v, SP_GRAD, l.gzx_off, n * 4 * l.H, true);
            if (l.multi) acc_add(v, SP_TMP, l.xch_off, 2 * (2 * l.H + 8 * l.H), true);
            break;
        }
        case K_COMB_F: case K_COMB_B: case K_COMB_F1: case K_COMB_F2: case K_COMB_B1: case K_COMB_B2: {
            // one launch each way, or the halves of a tiled plan (*1 writes the partial sums, *2 reads them back after the exchange)
            const CombineDesc& c = tab(combines)[s.first + i];
            const int64_t span = (int64_t)(c.Cn - 1) * (c.cs < 0 ? -c.cs : c.cs) + (int64_t)(c.rows - 1) * c.ld + c.cols;
            const int64_t lo = c.cs < 0 ? c.x_off + (int64_t)(c.Cn - 1) * c.cs : c.x_off;
            const int64_t n = (int64_t)c.rows * c.cols;
            const bool fwd = s.kind == K_COMB_F || s.kind == K_COMB_F1 || s.kind == K_COMB_F2, half2 = s.kind == K_COMB_F2 || s.kind == K_COMB_B2;
            acc_add(v, SP_WS, lo, span, false);
            acc_add(v, SP_TMP, c.part_off, COMBINE_MAXBLK * (COMBINE_MAXC + 1), !half2);
            if (fwd && s.kind != K_COMB_F1) { acc_add(v, SP_WS, c.out_off, n, true); acc_add(v, SP_TMP, c.stats_off, 64, true); }
            if (!fwd) { acc_add(v, SP_WS, c.out_off, n, false); acc_add(v, SP_GRAD, c.gout_off, n, false); }
            if (!fwd && s.kind != K_COMB_B1) {
                acc_add(v, SP_TMP, c.stats_off, 64, false);
                acc_add(v, SP_GRAD, lo - c.x_off + c.gx_off, span, true, true, span == (int64_t)c.Cn * n);
            }
            break;
        }
        case K_COPY_F: case K_COPY_B: {
            const CopyDesc& c = copies.host[s.first + i];
            const int64_t ss = (int64_t)(c.na - 1) * c.src_sa + (int64_t)(c.nb - 1) * c.src_sb + c.cols;
            const int64_t ds = (int64_t)(c.na - 1) * c.dst_sa + (int64_t)(c.nb - 1) * c.dst_sb + c.cols;
            if (s.kind == K_COPY_F) { acc_add(v, SP_WS, c.src_off, ss, false); acc_add(v, SP_WS, c.dst_off, ds, true); }
            else { acc_add(v, SP_GRAD, c.dst_off, ds, false); acc_add(v, SP_GRAD, c.src_off, ss, true, true, false); }
            break;
        }
        case K_FOLD: case K_SPREAD: {
            const FoldDesc& f = folds.host[s.first + i];
            const int64_t span = (int64_t)(f.nrows - 1) * f.row_stride + (int64_t)(f.ncols - 1) * f.col_stride + 1;
            acc_add(v, f.space, f.part_off, span, s.kind == K_SPREAD);
            acc_add(v, SP_TMP, f.sum_off, f.ncols, s.kind == K_FOLD);
            break;
        }
        case K_XCHG: {
            const Xchg& x = xchgs[s.first + i];
            acc_add(v, x.space, x.off, x.len, true);
            break;
        }
        case K_ROW_F: case K_ROW_B: {
            const RowLinDesc& r = tab(rowlins)[s.first + i];
            const int64_t nx = (int64_t)r.rows * r.kin, ny = (int64_t)r.rows * r.nout;
            acc_add(v, SP_WS, r.x_off, nx, false);
            acc_add(v, SP_WS, r.y_off, ny, s.kind == K_ROW_F);
            if (s.kind == K_ROW_B) {
                acc_add(v, SP_GRAD, r.y_off, ny, false);
                if (r.xgrad) acc_add(v, SP_GRAD, r.x_off, nx, true, true, true);
                acc_add(v, SP_TMP, r.slab_off, (int64_t)r.slab_stride * r.nblk, true);
            }
            break;
        }
        case K_ME_SQ: case K_ME_F: case K_ME_RED: case K_ME_B: {
            const NotesDesc& n = tab(notes)[s.first + i];
            const int64_t rows = (int64_t)n.C * n.Q, mel = (int64_t)n.Q * NF * NPN * n.W;
            const int64_t nparts = (int64_t)(n.C + 1) * n.nwc;
            acc_add(v, SP_WS, n.oct_off, rows * NOCT * n.W, false);
            acc_add(v, SP_WS, n.deg_off, rows * NDEG * n.W, false);
            if (s.kind == K_ME_SQ) acc_add(v, SP_TMP, n.part_off, nparts, true);
            else if (s.kind == K_ME_F) {
                acc_add(v, SP_TMP, n.part_off, nparts, false);
                acc_add(v, SP_TMP, n.stats_off, n.C + 1, true);
                acc_add(v, SP_WS, n.out_off, mel, true);
            } else if (s.kind == K_ME_RED) {
                acc_add(v, SP_WS, n.out_off, mel, false);
                acc_add(v, SP_GRAD, n.g_out_off, mel, false);
                acc_add(v, SP_TMP, n.part_off, nparts, true);
            } else {
                acc_add(v, SP_TMP, n.part_off, nparts, false);
                acc_add(v, SP_TMP, n.stats_off, n.C + 1, false);
                acc_add(v, SP_GRAD, n.g_out_off, mel, false);
                acc_add(v, SP_GRAD, n.g_oct_off, rows * NOCT * n.W, true);
                acc_add(v, SP_GRAD, n.g_deg_off, rows * NDEG * n.W, true);
                acc_add(v, SP_TMP, n.slab_off, (int64_t)n.slab_stride * n.nblk, true);
            }
            break;
        }
        case K_PSA_F: case K_PSA_B: {
            const NotesDesc& n = tab(notes)[s.first + i];
            const bool bwd = s.kind == K_PSA_B;
            const int64_t pos = (int64_t)n.C * n.Q * NF * NPN;
            const int ow = NOCT * 30, dw = NDEG * 30, outw = NPF;
            const int64_t mln = (int64_t)n.Q * NF * NPN * n.W;            // melody rows (melody_linear is applied inside the kernels)
            acc_add(v, SP_WS, n.rt_oct_off, (int64_t)n.Q * NF * ow, false);
            acc_add(v, SP_WS, n.rt_deg_off, (int64_t)n.Q * NF * dw, false);
            acc_add(v, SP_WS, n.it_oct_off, (int64_t)n.C * ow, false);
            acc_add(v, SP_WS, n.it_deg_off, (int64_t)n.C * dw, false);
            acc_add(v, SP_WS, n.mel_off, mln, false);
            acc_add(v, SP_WS, n.out_off, pos * outw, !bwd);
            if (bwd) {
                // (under MST_BF_LOSS_FUSED the upstream gradient is not read; declaring the read keeps the generic path safe)
                acc_add(v, SP_GRAD, n.g_out_off, pos * outw, false);
                acc_add(v, SP_WS, n.loss_saved_off, MST_LOSS_SAVED, false);
                acc_add(v, SP_WS, n.loss_gl_off, 64, false);
                acc_add(v, SP_GRAD, n.itp_oct_off, (int64_t)n.nblk * n.C * ow, true);      // per-workgroup partial gradients of it
                acc_add(v, SP_GRAD, n.itp_deg_off, (int64_t)n.nblk * n.C * dw, true);
                acc_add(v, SP_GRAD, n.rt_oct_off, (int64_t)n.Q * NF * ow, true);       // channel sums of dL/dz = gradient of rt
                acc_add(v, SP_GRAD, n.rt_deg_off, (int64_t)n.Q * NF * dw, true);
                acc_add(v, SP_GRAD, n.g_mel_off, mln, true);
                acc_add(v, SP_TMP, n.slab_off, (int64_t)n.slab_stride * n.nblk, true);
            }
            break;
        }
        }
    }
}

static bool conflicts(const std::vector<Acc>& a, const std::vector<Acc>& b) {
    for (const Acc& x : a)
        for (const Acc& y : b)
            if (x.space == y.space && (x.w || y.w) && x.lo < y.hi && y.lo < x.hi) return true;
    return false;
}

void mst_plan::schedule_pass(const std::vector<Step>& seq, std::vector<Step>& out, bool across_stages) {
    const int n = (int)seq.size();
    std::vector<std::vector<Acc>> acc(n);
    std::vector<int> level(n, 0);
    int maxlevel = 0;
    for (int i = 0; i < n; ++i) {
        accesses(seq[i], acc[i]);
        for (int j = 0; j < i; ++j)
            if (level[j] >= level[i] && conflicts(acc[i], acc[j])) level[i] = level[j] + 1;
        if (level[i] > maxlevel) maxlevel = level[i];
    }
    std::vector<char> done(n, 0);
    for (int lv = 0; lv <= maxlevel; ++lv) {
        const size_t lv_begin = out.size();
        for (int i = 0; i < n; ++i) {
            if (done[i] || level[i] != lv) continue;
            const Step& s0 = seq[i];
            const KindInfo& ki = KINDS[s0.kind];
            const bool mergeable = !opt.no_merge && ki.merge, is_lstm = ki.fam == F_LSTM;
            Step m = s0; m.count = 0; m.lvl = lv;
            std::vector<int> members;                       // indices into the per-kind descriptor vectors (one clip)
            for (int j = i; j < n; ++j) {
                if (done[j] || level[j] != lv) continue;
                const Step& s = seq[j];
                if (s.kind != s0.kind || (!across_stages && s.stage != s0.stage)) continue;
                // LSTM launches come in a register-resident (H <= 64), an L2 (<= 256) and a wide (<= 1024) flavour
                if (is_lstm && lstm_band(s.b) != lstm_band(s0.b)) continue;
                // ... and the multi-workgroup flavour is a kernel of its own (grid and hidden size fixed): never merged with another
                if (is_lstm && j != i && (lstms.host[s.first].multi || lstms.host[s0.first].multi)) continue;
                if (j != i && !mergeable) continue;
                done[j] = 1;
                for (int q = 0; q < s.count; ++q) members.push_back(s.first + q);
                m.stage |= s.stage;
                if (s.a > m.a) m.a = s.a;
                if (s.b > m.b) m.b = s.b;
            }
            // clip-major replication: clip k's copy of every member, relocated to clip k's workspace slices.
            // The W_hh transpose reads parameters only, so it runs once for all clips.
            // (the multi-workgroup flavour's K_LSTM_T step clears per-clip exchange tags instead: one copy per clip)
            // One-clip (32x32) GEMM launches dispatch their longest member first: a launch of more than one workgroup per CU runs in
            // rounds, and a member with a long dependent k chain that starts behind a round of short blocks makes the launch
            // as long as round + chain.  Stable, by descending k-tiles per workgroup (the kernel's own kchunk / KD), ties to the
            // accessor kinds that issue more per k-tile.  Members of one launch are independent, and slab offsets were fixed
            // when the model was emitted: only blk_begin and the block -> member table follow the order.
            if (ki.fam == F_GEMM && !mfma && !opt.no_merge) {
                auto ktiles = [&](int idx) {
                    const GemmDesc& g = gemms.host[idx];
                    const int kr = (g.K + g.ksplit - 1) / g.ksplit, kd = kr <= 32 ? 32 : (kr <= 64 ? 64 : 128);
                    return (kr + kd - 1) / kd;
                };
                auto dear = [&](int idx) {
                    switch (gemm_variant(gemms.host[idx])) {
                    case GV_CONV_FWD: case GV_CONV_DW: return 3;              // im2col / conv-gradient / permuted accessors
                    case GV_LIN_FWD_PERM: case GV_LIN_DW_PERM: return 2;
                    case GV_LIN_DW: case GV_LIN_DA: return 1;                 // two loads and the activation derivative per element
                    default: return 0;
                    }
                };
                std::stable_sort(members.begin(), members.end(), [&](int x, int y) {
                    const int kx = ktiles(x), ky = ktiles(y);
                    return kx != ky ? kx > ky : dear(x) > dear(y);
                });
            }
            const bool shared_T = s0.kind == K_LSTM_T && !lstms.host[s0.first].multi;
            const int reps = ki.per_clip && !shared_T ? K() : 1;
            if (ki.sched)
                with_sched_table(ki.fam, [&](auto& t) {
                    m.first = (int)t.sched.size();
                    for (int k = 0; k < reps; ++k)
                        for (int idx : members) t.sched.push_back(reloc(t.host[idx], k));
                });
            m.count = (int)members.size() * reps;
            if (ki.fam == F_GEMM) {
                for (int q = 0; q < m.count; ++q) {
                    GemmDesc& g = gemms.sched[m.first + q];
                    g.variant = gemm_variant(g);
                    if (g.fold_rows) {          // arena sizes are final now: clip strides of the folded reduction
                        g.acs = shift(g.A.space, 1); g.acs2 = (g.A.kind == OPK_ACTGRAD || g.A.kind == OPK_CONVGRAD) ? shift(g.A.space2, 1) : 0; g.bcs = shift(g.B.space, 1);
                        // the loader adds clip * stride as a 32-bit element offset
                        if ((uint64_t)std::max(g.acs, std::max(g.acs2, g.bcs)) * (uint64_t)K() > 0xFFFFFFFFull) err = MST_ERR_UNSUPPORTED;
                    }
                    if (g.clip_rows) {          // the clips become the rows: row stride = the clip stride of the operand's arena
                        g.M = K();
                        if (g.A.kind == OPK_DENSE) g.A.si = shift(g.A.space, 1);
                        else g.A.ld = (int32_t)shift(g.A.space, 1);              // OPK_ACTGRAD: dY and Y share the stride
                        g.out.ldc = (int32_t)shift(g.out.space, 1);
                        if ((uint64_t)act_top * (uint64_t)K() > 0x7FFFFFFFull) err = MST_ERR_UNSUPPORTED;     // 32-bit row offsets
                    }
                    const int kr = (g.K + g.ksplit - 1) / g.ksplit;
                    g.kdsel = kr <= 32 ? 0 : (kr <= 64 ? 1 : 2);
                    // tiles per workgroup (64x64 tiling): measured on MI355X at 64 clips per launch, runs of 2 / 4 / 8 tiles
                    // lost 7 / 22 / 33 % against one tile per workgroup (fewer, longer workgroups: worse balance over the
                    // 256 CUs than the saved per-workgroup latency buys), so the default stays 1; the option remains for experiments
                    g.run = (mfma && opt.gemm_run > 1) ? opt.gemm_run : 1;
                    if (g.variant < 0) err = MST_ERR_UNSUPPORTED;
                }
                // flat grid: a clip's block range concatenates its members' (tile, k-split) workgroups
                const int nm = (int)members.size();
                int total = 0;
                m.c = (int)s_gemm_owner.size();
                for (int q = 0; q < nm; ++q) {
                    const int nb = gemm_blocks(gemms.sched[m.first + q], mfma);
                    for (int k = 0; k < reps; ++k) gemms.sched[m.first + k * nm + q].blk_begin = total;
                    total += nb;
                    s_gemm_owner.insert(s_gemm_owner.end(), nb, q);
                }
                m.a = total; m.b = nm;        // blocks per clip, members per clip
            }
            if (m.kind == K_SEGRED) {    // same flat layout; m.b keeps the stage-2 block count, members = count / clips
                const int nm = (int)members.size();
                int total = 0;
                for (int q = 0; q < nm; ++q) {
                    const SegRedDesc& r0 = segreds.sched[m.first + q];
                    for (int k = 0; k < reps; ++k) segreds.sched[m.first + k * nm + q].blk_begin = total;
                    total += (r0.nidx * r0.nchunk * r0.width + 255) / 256;
                }
                m.a = total;
            }
            out.push_back(m);
        }
        // Steps of one level are independent, so the steps of the level that may ride (ride_slot) go to its GEMM launch (of the same
        // stage where stages may run separately): each to the first K_GEMM step whose slot is free.  The carried steps stay in the
        // list; run_step skips them.  `out` was empty when this pass began, so an index into it is the index into the finished list
        if (!mixes()) continue;
        for (size_t e = lv_begin; e < out.size(); ++e) {
            const int slot = ride_slot(out[e]);
            if (slot < 0) continue;
            for (size_t c = lv_begin; c < out.size(); ++c) {
                Step& g = out[c];
                if (g.kind != K_GEMM || (!across_stages && g.stage != out[e].stage) || g.rider[slot] >= 0) continue;
                g.rider[slot] = (int)e; out[e].carrier = (int)c;
                break;
            }
        }
    }
}

// The slot in which a scheduled step may ride a K_GEMM launch of its level (-1: it keeps its own launch)
int mst_plan::ride_slot(const Step& s) const {
    switch (s.kind) {
    case K_GATHER: return RIDE_GATHER;
    case K_SEGRED: return RIDE_SEGRED;            // stage 1; a second stage follows the carrier
    // combine steps where no site has more than 4 channels (the flavour whose registers fit gemm_kernel): a small site's whole
    // step, a large site's first phase
    case K_COMB_F: case K_COMB_B: return !mc4() ? -1 : (s.b != 0 ? RIDE_COMB_LARGE : RIDE_COMB_SMALL);
    // a backward LSTM step whose launch would take the one-wave kernel (not the grouped flavour) and whose W_hh fits the rider's
    // LDS slice beside the staged operands (the forward body beside it costs gemm_kernel two VGPRs: it keeps its launch)
    case K_LSTM_B: return (s.b <= LSTM_RIDE_H && lstm_small(s.count, s.a, s.b)) ? RIDE_LSTM : -1;
    default: return -1;
    }
}

// Gradient slots without a memset.  Walk a scheduled backward list in launch order and decide, for every writer that can
// accumulate (input-gradient GEMMs, segment reduces, combine backward, the row-wise Linear's dx), whether it is the FIRST
// writer of a dense, so far untouched range of the gradient arena — then it stores (=) and nothing has to be cleared — or
// lands on data written earlier in the pass — then it accumulates (+=).  Whatever is read, or accumulated into, without
// having been written before (rows of an LSTM output nobody consumes, strided / partially covered targets) goes on the
// zero list: the only ranges mst_zero_grads still clears.  (It was one memset of the whole arena: ~1 GB of writes per
// 64-clip pass, more than the algorithmic bytes of the pass.)
static bool covered(const std::vector<Acc>& have, int64_t lo, int64_t hi) {
    // is [lo, hi) inside the union of the ranges in `have`?  (few dozen ranges: quadratic sweep is fine)
    int64_t at = lo;
    bool moved = true;
    while (at < hi && moved) {
        moved = false;
        for (const Acc& a : have)
            if (a.lo <= at && a.hi > at) { at = a.hi; moved = true; }
    }
    return at >= hi;
}
static bool touches(const std::vector<Acc>& have, int64_t lo, int64_t hi) {
    for (const Acc& a : have) if (a.lo < hi && lo < a.hi) return true;
    return false;
}

void mst_plan::first_writers(std::vector<Step>& list, size_t begin, bool per_stage, std::vector<Acc>& zero) {
    std::vector<Acc> have;                               // ranges holding defined data at this point of the pass
    auto external = [&](const char* name) {              // written by the caller / the loss before the pass starts
        auto it = named.find(name);
        if (it != named.end()) have.push_back(Acc{SP_GRAD, it->second.off, it->second.off + MST_ALIGN_UP((int64_t)it->second.rows * it->second.cols), true});
    };
    for (const char* nm : {"pitched_pred", "unpitched_pred", "instruments_pred", "mode_pred", "bpm_pred"}) external(nm);
    if (per_stage) for (const char* nm : {"style", "melody", "rhythm"}) external(nm);      // seeded or cleared by the caller
    for (size_t si = begin; si < list.size(); ++si) {
        Step& m = list[si];
        // a kind that runs once for all clips has one descriptor per member (K_GEMM_FOLD: one first flag for a clips-as-rows dX)
        const int reps = KINDS[m.kind].per_clip ? K() : 1, nm = m.count / reps;
        for (int q = 0; q < nm; ++q) {
            std::vector<Acc> acc;
            Step one = m; one.first = m.first + q; one.count = 1;
            accesses(one, acc, true);
            for (const Acc& a : acc) {
                if (a.space != SP_GRAD || a.w) continue;
                if (!covered(have, a.lo, a.hi)) { Acc z = a; z.w = true; z.space = m.stage; zero.push_back(z); have.push_back(a); }
            }
            int first = 0;
            bool accum = false;
            for (const Acc& a : acc) {
                if (a.space != SP_GRAD || !a.w) continue;
                if (!a.accum) { if (a.dense) have.push_back(a); continue; }      // plain store of a dense range
                accum = true;
                if (a.dense && !touches(have, a.lo, a.hi)) { first = 1; have.push_back(a); }
                else if (!covered(have, a.lo, a.hi)) { Acc z = a; z.space = m.stage; zero.push_back(z); have.push_back(a); }
            }
            if (!accum) continue;                      // the flag belongs to the writers that can accumulate
            for (int k = 0, idx = m.first + q; k < reps; ++k, idx += nm) {
                switch (KINDS[m.kind].fam) {
                case F_GEMM: gemms.sched[idx].out.first = first; break;     case F_SEGRED: segreds.sched[idx].first = first; break;
                case F_COMB: combines.sched[idx].first = first; break;      case F_ROWLIN: rowlins.sched[idx].first = first; break;
                case F_COPY: copies.host[idx].first = first; break;         case F_LIN: lins.host[idx].first[per_stage ? 0 : 1] = first; break;
                }
            }
        }
    }
}

// Spread the launches of a scheduled whole-model list over 1 + N_SIDE streams along its dependency DAG (list scheduling): a
// launch depends on every earlier launch it shares memory with (any overlap with a write on either side: conflicts()).  In list
// order, each launch goes to the stream where it can start first under a simple cost model (a launch on the stream of the
// predecessor it waits for longest starts right behind it; a dependency that crosses streams costs an event wait, measured
// ~5 us per edge inside a replayed hipGraph against ~2 us for a same-stream boundary — so the model is reluctant to cross).
// Cross-stream dependencies become (signal, wait) pairs: the producer records an event slot behind it, the consumer's stream
// waits for it; waits already implied by stream order or by an earlier wait are dropped (vector clocks).  The result is checked:
// every conflicting pair must be ordered by stream order and waits, else the plan keeps one stream.
bool mst_plan::assign_streams(std::vector<Step>& L) {
    const int n = (int)L.size(), NS = 1 + N_SIDE;
    std::vector<std::vector<Acc>> acc(n);
    for (int i = 0; i < n; ++i) accesses(L[i], acc[i], true);
    auto dur = [&](const Step& st) {           // rough one-clip durations in us (profiles/: pass_timeline_one_clip)
        switch (st.kind) {
        case K_LSTM_F: case K_LSTM_B: return lstms.sched[st.first].multi ? 30.0 : 15.0;
        case K_ME_F: case K_ME_B: case K_PSA_F: case K_PSA_B: return 18.0;
        case K_GEMM: case K_GEMM_FOLD: return st.count > 8 ? 10.0 : 5.0;
        case K_SEGRED: return 9.0;
        default: return 5.0;
        }
    };
    const double EDGE_IN = 2.0, EDGE_X = 6.0;
    std::vector<double> fin(n, 0.0);
    std::vector<int> str(n, 0);
    double ready[1 + N_SIDE] = {};
    // clock[i][r]: the latest launch index on stream r known to be complete when launch i starts (through stream order and waits)
    std::vector<std::array<int, 1 + N_SIDE>> clock(n);
    int tail[1 + N_SIDE]; for (int q = 0; q < NS; ++q) tail[q] = -1;
    for (int i = 0; i < n; ++i) {
        std::vector<int> preds;
        for (int j = 0; j < i; ++j) if (conflicts(acc[i], acc[j])) preds.push_back(j);
        int best = 0; double best_start = 1e30;
        for (int q = 0; q < NS; ++q) {
            double start = ready[q];
            for (int j : preds) start = std::max(start, fin[j] + (str[j] == q ? 0.0 : EDGE_X));
            if (start < best_start - 1e-9) { best_start = start; best = q; }
        }
        const int q = best;
        str[i] = q; L[i].chain = q;
        fin[i] = best_start + dur(L[i]) + EDGE_IN; ready[q] = fin[i];
        // what is known complete when i starts: its stream's tail (and what that knew), then the waits
        std::array<int, 1 + N_SIDE> ck; ck.fill(-1);
        if (tail[q] >= 0) { ck = clock[tail[q]]; ck[q] = tail[q]; }
        int need[1 + N_SIDE]; for (int r = 0; r < NS; ++r) need[r] = -1;
        for (int j : preds) if (str[j] != q && j > ck[str[j]]) need[str[j]] = std::max(need[str[j]], j);
        int nw = 0;
        for (int r = 0; r < NS; ++r) {
            if (need[r] < 0) continue;
            const int j = need[r];
            if (L[j].signal < 0) { if (n_signals >= N_EVENTS) return false; L[j].signal = n_signals++; }
            L[i].wait[nw++] = L[j].signal;
            for (int t = 0; t < NS; ++t) ck[t] = std::max(ck[t], clock[j][t]);
            ck[r] = std::max(ck[r], j);
        }
        clock[i] = ck; tail[q] = i;
    }
    // check: every conflicting pair (j < i) is ordered
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j)
            if (conflicts(acc[i], acc[j]) && !(str[j] == str[i] || clock[i][str[j]] >= j)) return false;
    return true;
}

void mst_plan::schedule() {
    // Two GEMM tilings, both on v_mfma_f32_32x32x2_f32: few clips per launch are latency-bound and want many small
    // workgroups with a short k chain (32x32 tiles, 16 waves split the k-tile); from about six clips per launch on
    // the launches fill the chip and the 64x64-tile kernel (16-byte tile loads) wins (measured crossover between 4 and 8
    // clips: 2475 vs 2306 clip-it/s at 4, 3060 vs 3340 at 8).  mst_plan_options.gemm_tile = 32 | 64 forces one (experiments, tests).
    mfma = opt.gemm_tile == 64 ? 1 : (opt.gemm_tile == 32 ? 0 : (K() >= 6));
    std::vector<Step> fwd, bwd;
    for (auto& op : ops) for (auto s : op.fwd) { s.stage = op.stage; fwd.push_back(s); }
    for (size_t i = ops.size(); i-- > 0;) for (auto s : ops[i].bwd) { s.stage = ops[i].stage; bwd.push_back(s); }
    schedule_pass(fwd, sched[0], false);
    schedule_pass(bwd, sched[1], false);
    // mst_plan_options.branches: the whole-model lists' launches are spread over streams along the dependency DAG
    branches = opt.branches == 1 && !tiled();
    schedule_pass(fwd, sched_all[0], true);
    schedule_pass(bwd, sched_all[1], true);
    std::vector<Acc> zs, za;
    first_writers(sched[1], 0, true, zs);
    first_writers(sched_all[1], 0, false, za);
    if (branches && !(assign_streams(sched_all[0]) && assign_streams(sched_all[1]))) {
        branches = false;
        for (int ps = 0; ps < 2; ++ps) for (Step& st : sched_all[ps]) { st.chain = -1; st.signal = -1; st.wait[0] = st.wait[1] = st.wait[2] = -1; }
    }
    // zero lists -> chunks of <= 16 K floats (one workgroup each); Acc.space carries the stage of the step that needs it
    auto chunks = [&](const std::vector<Acc>& z, int stage_mask, std::vector<ZeroChunk>& out) {
        for (const Acc& a : z) {
            if (!(a.space & stage_mask)) continue;
            for (int64_t at = a.lo; at < a.hi; at += 16384) out.push_back(ZeroChunk{at, (int32_t)std::min<int64_t>(16384, a.hi - at), 0});
        }
    };
    for (int st = 0; st < 3; ++st) chunks(zs, 1 << st, zero_stage[st]);
    chunks(za, MST_STAGE_ALL, zero_all);
    // one-clip plans: the exchange tags of the multi-workgroup LSTM ride on the same launch (the scratch arena follows the
    // gradient arena, so a chunk can address it); mst_train_iteration then skips the separate clear
    if (K() == 1)
        for (const LstmDesc& l : lstms.host)
            if (l.multi) { zero_all.push_back(ZeroChunk{arena(SP_TMP) - arena(SP_GRAD) + l.xch_off, (int32_t)(2 * (2 * l.H + 8 * l.H)), 0}); tags_in_zero = true; }
    find_zero_ride();
    if (!tiled()) return;
    // ---- one train iteration of a tiled plan as phases that end at an exchange
    {   // loss partial sums (7 per note tensor, one row per workgroup) -> 16 floats that the ranks sum
        const bool U = d.has_unpitched != 0;
        loss_sum_off = tmp(16);
        FoldDesc f{}; f.space = SP_TMP; f.part_off = loss_scratch; f.nrows = loss_blocks(loss.np); f.row_stride = 8; f.ncols = 7; f.col_stride = 1;
        f.sum_off = loss_sum_off;
        loss_fold[0] = (int)folds.host.size(); folds.host.push_back(f);
        f.part_off = loss_scratch + (mst_loss_scratch_floats() - 64) / 2; f.nrows = U ? loss_blocks(loss.nu) : 1; f.sum_off = loss_sum_off + 8;
        loss_fold[1] = (int)folds.host.size(); folds.host.push_back(f);
    }
    auto mk = [](int what, int pass, int begin, int end) { Phase ph{}; ph.what = what; ph.pass = pass; ph.begin = begin; ph.end = end; ph.nx = 0; return ph; };
    // An exchange is DEFERRED past every following step that does not touch its range (the list is a valid order, and such a step
    // cannot depend on what the exchange delivers): it joins the group of pending exchanges, and the phase is cut only in front of
    // the first step that reads or writes a pending range — all pending exchanges then travel as one collective.  13 ranges per
    // iteration become the number of true dependency points between exchanged data and its consumers.
    auto split = [&](int pass) {
        const std::vector<Step>& L = sched_all[pass];
        int begin = 0;
        Phase cur = mk(0, pass, 0, 0);
        auto touches_pending = [&](const Step& st) {
            if (!cur.nx) return false;
            std::vector<Acc> acc;
            accesses(st, acc, true);
            for (int q = 0; q < cur.nx; ++q) {
                const Xchg& x = xchgs[cur.xchg[q]];
                for (const Acc& a : acc)
                    if (a.space == x.space && a.lo < x.off + x.len && x.off < a.hi) return true;
            }
            return false;
        };
        for (int i = 0; i < (int)L.size(); ++i) {
            const bool is_x = L[i].kind == K_XCHG;
            if ((is_x && cur.nx == MST_MAX_XCHG) || (!is_x && touches_pending(L[i]))) {
                cur.begin = begin; cur.end = i;          // steps [begin, i) run (exchange steps among them are skipped), then the exchanges
                phases.push_back(cur);
                begin = i; cur = mk(0, pass, 0, 0);
            }
            if (is_x) cur.xchg[cur.nx++] = L[i].first;
        }
        cur.begin = begin; cur.end = (int)L.size();
        phases.push_back(cur);                            // (a trailing group of exchanges, if any, is delivered after the last step)
    };
    split(0);
    const int lx = (int)xchgs.size();
    xchgs.push_back(Xchg{SP_TMP, loss_sum_off, 16});
    { Phase ph = mk(1, 0, 0, 0); ph.nx = 1; ph.xchg[0] = lx; phases.push_back(ph); }
    phases.push_back(mk(2, 0, 0, 0));
    split(1);
}

void mst_plan::find_zero_ride() {
    zero_ride = -1;
    if (!mixes() || zero_all.empty()) return;
    const std::vector<Step>& L = sched_all[0];
    int first = -1;
    for (int i = 0; i < (int)L.size() && first < 0; ++i) {
        if (L[i].carrier >= 0) continue;
        if (tags_in_zero && L[i].kind == K_LSTM_T && lstms.sched[L[i].first].multi) continue;      // skipped: its only job was the clear
        first = i;
    }
    if (first < 0 || L[first].kind != K_GEMM) return;
    // everything in absolute workspace floats (arena)
    std::vector<Acc> acc;
    accesses(L[first], acc, true);
    // its riders are every carried step of its level: a whole-model list of a plan that mixes merges a level's K_GEMM steps into one
    for (const int r : L[first].rider) if (r >= 0) accesses(L[r], acc, true);
    for (const Acc& a : acc) {
        const int64_t ab = arena(a.space);
        if (ab < 0) continue;                        // parameters and the borrowed inputs: not in the workspace
        for (int k = 0; k < K(); ++k)
            for (const ZeroChunk& c : zero_all) {
                const int64_t lo = arena(SP_GRAD) + shift(SP_GRAD, k) + c.off;
                if (ab + a.lo < lo + c.len && lo < ab + a.hi) return;
            }
    }
    zero_ride = first;
}

// two column blocks of one row-major matrix (row pitch ld), given by the offsets of their first elements from the matrix's
// element (0, 0): do they share no element?  (both start in row 0 or any row: only the column intervals matter)
static bool slab_columns_disjoint(int64_t off_x, int width_x, int64_t off_y, int width_y, int ld) {
    const int64_t cx = off_x % ld, cy = off_y % ld;
    if (cx + width_x > ld || cy + width_y > ld) return false;       // a block that wraps a row is not a column block
    return cx + width_x <= cy || cy + width_y <= cx;
}
extern "C" int32_t mst_debug_slab_columns_disjoint(int64_t off_x, int32_t width_x, int64_t off_y, int32_t width_y, int32_t ld) {
    return slab_columns_disjoint(off_x, width_x, off_y, width_y, ld) ? 1 : 0;
}

int mst_plan::upload() {
    int e = 0;
    e |= gemms.upload(); e |= gathers.upload(); e |= segreds.upload(); e |= lstms.upload();
    e |= combines.upload(); e |= notes.upload(); e |= rowlins.upload();
    e |= up(s_gemm_owner, &d_gemm_owner);
    e |= copies.upload(); e |= folds.upload(); e |= up(zero_fwd, &d_zero_fwd);      // (convs and lins go by value)
    for (int st = 0; st < 3; ++st) e |= up(zero_stage[st], &d_zero_stage[st]);
    e |= up(zero_all, &d_zero_all);
    for (int s = 0; s < 3; ++s) {
        for (auto& ent : slabs[s]) { ent.reps = ent.single ? 1 : K(); ent.rep_stride = tmp_top; }
        e |= up(slabs[s], &d_slabs[s]);
        for (size_t i = 0; i < slabs[s].size(); ++i)
            for (int st = 0; st < slabs[s][i].count; st += 64) slab_blocks[s].push_back(SlabBlock{(int)i, st});
        e |= up(slab_blocks[s], &d_slab_blocks[s]);
    }
    {   // one list for the whole-model backward; two workgroups must never add into the same parameter element concurrently
        std::vector<std::pair<int64_t, int64_t>> spans;
        for (int s = 0; s < 3; ++s)
            for (auto& ent : slabs[s]) {
                const int64_t hi = ent.width > 0 ? ent.dst + (int64_t)(ent.count / ent.width - 1) * ent.dst_ld + ent.width : ent.dst + ent.count;
                spans.push_back({ent.dst, hi});
                slabs_all.push_back(ent);
            }
        // entries whose bounding spans overlap are disjoint only as column blocks of the SAME parameter matrix (same base, same
        // row pitch) with disjoint column ranges, columns counted from the matrix's own first element
        slabs_all_ok = true;
        for (size_t i = 0; i < slabs_all.size() && slabs_all_ok; ++i)
            for (size_t j = i + 1; j < slabs_all.size() && slabs_all_ok; ++j) {
                const SlabEntry& x = slabs_all[i]; const SlabEntry& y = slabs_all[j];
                if (spans[i].second <= spans[j].first || spans[j].second <= spans[i].first) continue;
                slabs_all_ok = x.width > 0 && y.width > 0 && x.dst_ld == y.dst_ld && x.base == y.base &&
                               slab_columns_disjoint(x.dst - x.base, x.width, y.dst - y.base, y.width, x.dst_ld);
            }
        for (size_t i = 0; i < slabs_all.size(); ++i)
            for (int st = 0; st < slabs_all[i].count; st += 64) slab_blocks_all.push_back(SlabBlock{(int)i, st});
        e |= up(slabs_all, &d_slabs_all);
        e |= up(slab_blocks_all, &d_slab_blocks_all);
    }
    return e ? MST_ERR_ALLOC : MST_OK;
}

extern "C" int32_t mst_widths_supported(const mst_dims* d) {
    if (!dims_ok(d)) return MST_ERR_ARG;
    return widths_supported(mst_sizes(*d)) ? MST_OK : MST_ERR_UNSUPPORTED;
}

extern "C" mst_plan* mst_plan_create(const mst_dims* d, int32_t* status) { return mst_plan_create_ex(d, nullptr, status); }

extern "C" mst_plan* mst_plan_create_ex(const mst_dims* d, const mst_plan_options* opt, int32_t* status) {
    int32_t dummy; if (!status) status = &dummy;
    if (!dims_ok(d)) { *status = MST_ERR_ARG; return nullptr; }
    if (opt && ((opt->gemm_tile != 0 && opt->gemm_tile != 32 && opt->gemm_tile != 64) || opt->gemm_run < 0 || opt->gemm_run > 64)) { *status = MST_ERR_ARG; return nullptr; }
    if (opt && (opt->lstm_flavour < 0 || opt->lstm_flavour > 2 || opt->dense_flavour < 0 || opt->dense_flavour > 2 || opt->branches < 0 || opt->branches > 1)) { *status = MST_ERR_ARG; return nullptr; }
    if (opt && (opt->tile_rows < 0 || opt->tile_r0 < 0 || (opt->tile_rows > 0 && (opt->tile_r0 + opt->tile_rows > d->R || d->clips > 1)))) {
        *status = MST_ERR_ARG; return nullptr;
    }
    mst_plan* p = new mst_plan();
    if (opt) p->opt = *opt;
    p->d = *d; p->z = mst_sizes(*d);
    if (p->d.clips < 1) p->d.clips = 1;
    build_params(*d, p->z, p->pt);
    p->build();
    if (!p->err) { p->resolve_loss(); p->schedule(); }
    if (p->err) { *status = p->err; delete p; return nullptr; }
    int e = p->upload();
    if (e) { *status = e; mst_plan_destroy(p); return nullptr; }
    *status = MST_OK;
    return p;
}

extern "C" void mst_plan_destroy(mst_plan* p) {
    if (!p) return;
    p->gemms.release(); p->gathers.release(); p->segreds.release(); p->lstms.release(); p->combines.release(); p->notes.release();
    p->rowlins.release(); p->copies.release(); p->folds.release();
    hipFree(p->d_gemm_owner); hipFree(p->d_zero_all); hipFree(p->d_zero_fwd);
    for (int st = 0; st < 3; ++st) hipFree(p->d_zero_stage[st]);
    for (int s = 0; s < 3; ++s) { hipFree(p->d_slabs[s]); hipFree(p->d_slab_blocks[s]); }
    hipFree(p->d_slabs_all); hipFree(p->d_slab_blocks_all);
    for (mst_plan::SideSet& q : p->sides) {
        if (q.ev_fork) hipEventDestroy(q.ev_fork);
        for (int i = 0; i < mst_plan::N_SIDE; ++i) { if (q.ev_join[i]) hipEventDestroy(q.ev_join[i]); if (q.side[i]) hipStreamDestroy(q.side[i]); }
        for (hipEvent_t e : q.ev) if (e) hipEventDestroy(e);
    }
    delete p;
}

extern "C" int64_t mst_plan_workspace_floats(const mst_plan* p) { return p ? (int64_t)p->K() * (2 * p->act_top + p->tmp_top) : MST_ERR_ARG; }

extern "C" int32_t mst_plan_gemm_tile(const mst_plan* p) { return p ? (p->mfma ? 64 : 32) : MST_ERR_ARG; }

extern "C" int32_t mst_plan_layout(const mst_plan* p, int64_t out[4]) {
    if (!p || !out) return MST_ERR_ARG;
    out[0] = p->K(); out[1] = p->act_top; out[2] = p->tmp_top; out[3] = p->arena(SP_GRAD);
    return MST_OK;
}

extern "C" int32_t mst_plan_tensor(const mst_plan* p, const char* name, int64_t* off, int64_t* goff, int64_t* numel) {
    if (!p || !name) return MST_ERR_ARG;
    auto it = p->named.find(name);
    if (it == p->named.end()) return MST_ERR_ARG;
    if (off) *off = it->second.off;
    if (goff) *goff = p->arena(SP_GRAD) + it->second.off;
    if (numel) *numel = (int64_t)it->second.rows * it->second.cols;
    return MST_OK;
}

// The steps of pass (mask, backward), in list order: what the report and instrumentation entry points index (run_pass filters in place)
static std::vector<const Step*> steps_of(const mst_plan* p, int mask, int backward) {
    std::vector<const Step*> steps;
    for (auto& s : p->list(mask, backward)) if (s.stage & mask) steps.push_back(&s);
    return steps;
}

extern "C" int32_t mst_plan_launch_count(const mst_plan* p, int32_t mask, int32_t backward) {
    if (!p) return MST_ERR_ARG;
    int n = 0;
    for (const Step* s : steps_of(p, mask, backward))
        n += (s->carrier >= 0 ? 0 : 1) + (second_stage(*s) ? 1 : 0);          // a carried step's first stage is part of its carrier's launch
    if (backward) for (int s = 0; s < 3; ++s) if ((mask >> s) & 1) n += 1;
    return n;
}

static Bases make_bases(const mst_plan* p, const float* params, float* gparams, float* ws, const float* pitched,
                        const float* unpitched) {
    Bases b;
    b.p[SP_WS] = ws; b.p[SP_PAR] = const_cast<float*>(params); b.p[SP_GPAR] = gparams;
    b.p[SP_EXT0] = const_cast<float*>(pitched); b.p[SP_EXT1] = const_cast<float*>(unpitched);
    b.p[SP_GRAD] = ws + p->arena(SP_GRAD); b.p[SP_TMP] = ws + p->arena(SP_TMP);
    b.flags = 0;
    return b;
}

// L: the scheduled list `s` is a step of (a carrier's riders are indices into it)
// with_zero: the launch also clears the whole-model zero list (the K_GEMM step mst_plan::zero_ride names, in mst_train_iteration)
static int run_step(const mst_plan* p, const std::vector<Step>& L, const Step& s, const Bases& b, hipStream_t st, bool with_zero = false) {
    if (s.carrier >= 0) return 0;         // launched by its carrier
    switch (s.kind) {
    case K_GEMM: case K_GEMM_FOLD: {
        // an empty slot reads as a step without members: first 0, count 0, a 0, b 0
        static const Step none{-1, 0, 0, 0, 0, 0};
        auto rider = [&](int slot) -> const Step& { return s.rider[slot] >= 0 ? L[s.rider[slot]] : none; };
        const Step &lstm = rider(RIDE_LSTM), &small = rider(RIDE_COMB_SMALL), &large = rider(RIDE_COMB_LARGE), &seg = rider(RIDE_SEGRED), &gat = rider(RIDE_GATHER);
        const int clips = s.count / s.b, K = p->K();      // a rider's members per clip: count / K
        // segment reduce: a = 256-lane groups per clip; gather: a = most rows of a member -> workgroups per member
        GemmRiders r{p->segreds.dev + seg.first, seg.count / K, seg.a, p->gathers.dev + gat.first, gat.count / K,
                     std::min(512, (gat.a + GATHER_RIDER_ROWS - 1) / GATHER_RIDER_ROWS)};
        // combine: a = most 256-lane groups of a site, four per workgroup of a large site
        if (small.count) r.comb[0] = {p->combines.dev + small.first, small.count / K, 1, small.kind == K_COMB_B ? COMB_RIDE_SMALL_B : COMB_RIDE_SMALL_F};
        if (large.count) r.comb[1] = {p->combines.dev + large.first, large.count / K, (large.a + 3) / 4, large.kind == K_COMB_B ? COMB_RIDE_REDUCE : COMB_RIDE_SUMSQ};
        // small backward LSTM: a = most sequences of a member, one per wave
        if (lstm.count) { r.lstms = p->lstms.dev + lstm.first; r.lstm_members = lstm.count / K; r.lstm_blocks = (lstm.a + GEMM_THREADS / 64 - 1) / (GEMM_THREADS / 64); }
        if (with_zero) { r.zero = p->d_zero_all; r.zero_chunks = (int)p->zero_all.size(); r.zero_stride = p->act_top; }
        int e = launch_gemm(p->gemms.dev + s.first, p->d_gemm_owner + s.c, s.b, s.a, clips, p->mfma, b, st, &r);
        // second stages of what it carried: directly behind the carrier
        if (!e && second_stage(seg)) e = launch_segred2(p->segreds.dev + seg.first, seg.count / K * clips, seg.b, b, st);
        if (!e && second_stage(large))
            e = launch_combine_phase(p->combines.dev + large.first, large.a, large.kind == K_COMB_B ? 3 : 1, b, st, large.count / K * clips, 1, 1);
        return e;
    }
    case K_GATHER: return launch_gather(p->gathers.dev + s.first, s.count, s.a, b, st);
    case K_SEGRED: return launch_segred(p->segreds.dev + s.first, s.count / p->K(), s.a, p->K(), s.b, b, st);
    case K_LSTM_T: return launch_lstm_transpose(p->lstms.dev + s.first, s.count, s.b, p->lstms.sched[s.first].multi, b, st);
    case K_LSTM_F: return launch_lstm_fwd(p->lstms.dev + s.first, s.count, s.a, s.b, p->lstms.sched[s.first].multi, p->lstm_small_on, b, st);
    case K_LSTM_B: return launch_lstm_bwd(p->lstms.dev + s.first, s.count, s.a, s.b, p->lstms.sched[s.first].multi, p->lstm_small_on, b, st);
    case K_COMB_F: return launch_combine_fwd(p->combines.dev + s.first, s.count, s.a, s.b == 0 ? (p->mc4() ? 2 : 1) : 0, p->mc4(), b, st);
    case K_COMB_B: return launch_combine_bwd(p->combines.dev + s.first, s.count, s.a, s.b == 0 ? (p->mc4() ? 2 : 1) : 0, p->mc4(), b, st);
    case K_COMB_F1: return launch_combine_phase(p->combines.dev + s.first, s.a, 0, b, st, 1, p->mc4());
    case K_COMB_F2: return launch_combine_phase(p->combines.dev + s.first, s.a, 1, b, st, 1, p->mc4());
    case K_COMB_B1: return launch_combine_phase(p->combines.dev + s.first, s.a, 2, b, st, 1, p->mc4());
    case K_COMB_B2: return launch_combine_phase(p->combines.dev + s.first, s.a, 3, b, st, 1, p->mc4());
    case K_COPY_F: return launch_copy_rows(p->copies.dev + s.first, p->copies.host[s.first], 0, b, st);
    case K_COPY_B: return launch_copy_rows(p->copies.dev + s.first, p->copies.host[s.first], 1, b, st);
    case K_FOLD: return launch_fold(p->folds.dev + s.first, 0, b, st);
    case K_SPREAD: return launch_fold(p->folds.dev + s.first, 1, b, st);
    case K_XCHG: return MST_ERR_UNSUPPORTED;        // a tiled plan runs through mst_tiled_phase, which stops at exchanges
    case K_LIN_F: case K_LIN_A: case K_LIN_W: {
        LinDesc l = p->lins.host[s.first];
        l.x_cs = p->shift(l.x_space, 1); l.y_cs = p->act_top; l.gx_cs = p->act_top;
        if (s.kind == K_LIN_F) return launch_lin_fwd(l, b, st);
        if (s.kind == K_LIN_W) return launch_lin_dw(l, b, st);
        return launch_lin_dx(l, b, l.first[(b.flags & MST_BF_ALL_STAGES) ? 1 : 0], st);
    }
    case K_CONV_P: { ConvDesc c = p->convs.host[s.first]; c.clip_stride = p->act_top; return launch_conv_prep(c, b, st); }
    case K_CONV_F: { ConvDesc c = p->convs.host[s.first]; c.clip_stride = p->act_top; return launch_conv_fwd(c, b, st); }
    case K_CONV_W: { ConvDesc c = p->convs.host[s.first]; c.clip_stride = p->act_top; return launch_conv_dw(c, b, st); }
    case K_ROW_F: return launch_rowlin_fwd(p->rowlins.dev + s.first, p->rowlins.sched[s.first], s.count, b, st);
    case K_ROW_B: return launch_rowlin_bwd(p->rowlins.dev + s.first, p->rowlins.sched[s.first], s.count, b, st);
    case K_ME_SQ: return launch_me_sumsq(p->notes.dev + s.first, p->notes.sched[s.first], s.count, b, st);
    case K_ME_RED: return launch_me_bwd_reduce(p->notes.dev + s.first, p->notes.sched[s.first], s.count, b, st);
    case K_ME_F: return launch_me_notes_fwd(p->notes.dev + s.first, p->notes.sched[s.first], s.count, b, st);
    case K_ME_B: return launch_me_notes_bwd(p->notes.dev + s.first, p->notes.sched[s.first], s.count, b, st);
    case K_PSA_F: return launch_psa_notes_fwd(p->notes.dev + s.first, p->notes.sched[s.first], s.count, b, st);
    case K_PSA_B: return launch_psa_notes_bwd(p->notes.dev + s.first, p->notes.sched[s.first], s.count, b, st);
    }
    return MST_ERR_ARG;
}

// Run one pass (a scheduled list filtered by stage) on the caller's stream.
static int run_pass(const mst_plan* p, const std::vector<Step>& list, int mask, const Bases& b0, hipStream_t main, bool tags_cleared = false,
                    int zero_step = -1 /* index of the step whose launch also clears the zero list */) {
    Bases b = b0;
    if (mask == MST_STAGE_ALL) b.flags |= MST_BF_ALL_STAGES;            // p->list(mask, .) is the whole-model list then
    auto runs = [&](const Step& s) {
        if (!(s.stage & mask)) return false;
        if (tags_cleared && s.kind == K_LSTM_T && p->lstms.sched[s.first].multi) return false;     // its only job was the clear
        return true;
    };
    // Streams (plans with `branches`, whole-model lists): launch s goes to stream s.chain (0 = the caller's, c = side stream c - 1)
    // behind the waits assign_streams gave it; a side stream's first launch of the pass also waits for the caller's stream (fork),
    // and the caller's stream waits for every side stream at the end (join) — parallel branches once captured into a hipGraph.
    mst_plan::SideSet* ss = (p->branches && mask == MST_STAGE_ALL) ? p->side_set(main) : nullptr;
    bool forked = false, used[mst_plan::N_SIDE] = {};
    for (auto& s : list) {
        if (!runs(s)) continue;
        hipStream_t st = main;
        if (ss) {
            if (s.chain > 0) {
                const int c = s.chain - 1;
                if (!forked) { if (hipEventRecord(ss->ev_fork, main) != hipSuccess) return MST_ERR_LAUNCH; forked = true; }
                if (!used[c]) { if (hipStreamWaitEvent(ss->side[c], ss->ev_fork, 0) != hipSuccess) return MST_ERR_LAUNCH; used[c] = true; }
                st = ss->side[c];
            }
            for (int w = 0; w < 3; ++w)
                if (s.wait[w] >= 0 && hipStreamWaitEvent(st, ss->ev[s.wait[w]], 0) != hipSuccess) return MST_ERR_LAUNCH;
        }
        int e = run_step(p, list, s, b, st, zero_step >= 0 && &s == &list[zero_step]);
        if (e) return e < 0 ? e : MST_ERR_LAUNCH;
        if (ss && s.signal >= 0 && hipEventRecord(ss->ev[s.signal], st) != hipSuccess) return MST_ERR_LAUNCH;
    }
    if (ss)
        for (int c = 0; c < mst_plan::N_SIDE; ++c)
            if (used[c] && (hipEventRecord(ss->ev_join[c], ss->side[c]) != hipSuccess || hipStreamWaitEvent(main, ss->ev_join[c], 0) != hipSuccess)) return MST_ERR_LAUNCH;
    return MST_OK;
}

extern "C" int32_t mst_forward(const mst_plan* p, int32_t mask, const float* params, float* ws, const float* pitched,
                               const float* unpitched, mst_stream stream) {
    if (!p || !params || !ws) return MST_ERR_ARG;
    if ((mask & MST_STAGE_EXTRACT) && (!pitched || (p->d.has_unpitched && !unpitched))) return MST_ERR_ARG;
    const Bases b = make_bases(p, params, nullptr, ws, pitched, unpitched);
    return run_pass(p, p->list(mask, 0), mask, b, (hipStream_t)stream);
}

extern "C" int32_t mst_plan_status(const mst_plan* p, float* ws, int32_t clear, int32_t* status, mst_stream stream) {
    if (!p || !ws || !status) return MST_ERR_ARG;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) return MST_ERR_LAUNCH;
    int32_t word = 0;
    if (hipMemcpy(&word, ws + p->status_off, sizeof(word), hipMemcpyDeviceToHost) != hipSuccess) return MST_ERR_LAUNCH;
    *status = word;
    if (clear && word) {
        const int32_t zero = 0;
        if (hipMemcpy(ws + p->status_off, &zero, sizeof(zero), hipMemcpyHostToDevice) != hipSuccess) return MST_ERR_LAUNCH;
    }
    return MST_OK;
}

extern "C" int32_t mst_zero_grads(const mst_plan* p, int32_t mask, float* ws, mst_stream stream) {
    if (!p || !ws) return MST_ERR_ARG;
    // only the ranges the first-writer analysis could not prove written before they are read / accumulated into
    float* g = ws + p->arena(SP_GRAD);
    if ((mask & MST_STAGE_ALL) == MST_STAGE_ALL)
        return launch_zero(p->d_zero_all, (int)p->zero_all.size(), p->K(), g, p->act_top, (hipStream_t)stream) ? MST_ERR_LAUNCH : MST_OK;
    for (int s = 0; s < 3; ++s) {
        if (!((mask >> s) & 1)) continue;
        if (launch_zero(p->d_zero_stage[s], (int)p->zero_stage[s].size(), p->K(), g, p->act_top, (hipStream_t)stream)) return MST_ERR_LAUNCH;
    }
    return MST_OK;
}

static int32_t backward_impl(const mst_plan* p, int32_t mask, const float* params, float* gparams, float* ws,
                             const float* pitched, const float* unpitched, mst_stream stream, int32_t flags) {
    if (!p || !params || !gparams || !ws) return MST_ERR_ARG;
    if ((mask & MST_STAGE_EXTRACT) && (!pitched || (p->d.has_unpitched && !unpitched))) return MST_ERR_ARG;
    Bases b = make_bases(p, params, gparams, ws, pitched, unpitched);
    b.flags = flags;
    {
        int e = run_pass(p, p->list(mask, 1), mask, b, (hipStream_t)stream);
        if (e) return e;
    }
    if ((mask & MST_STAGE_ALL) == MST_STAGE_ALL && p->slabs_all_ok)      // whole model: the three stages' reductions in one launch
        return launch_slab_reduce(p->d_slabs_all, p->d_slab_blocks_all, (int)p->slab_blocks_all.size(), b, (hipStream_t)stream) ? MST_ERR_LAUNCH : MST_OK;
    for (int s = 2; s >= 0; --s) {
        if (!((mask >> s) & 1)) continue;
        if (launch_slab_reduce(p->d_slabs[s], p->d_slab_blocks[s], (int)p->slab_blocks[s].size(), b, (hipStream_t)stream))
            return MST_ERR_LAUNCH;
    }
    return MST_OK;
}

extern "C" int32_t mst_backward(const mst_plan* p, int32_t mask, const float* params, float* gparams, float* ws,
                                const float* pitched, const float* unpitched, mst_stream stream) {
    return backward_impl(p, mask, params, gparams, ws, pitched, unpitched, stream, 0);
}

// The loss kernels with their operands from the plan's LossOps.  LOSS_WHOLE: every clip's losses in one go; a tiled plan runs the
// two halves instead, around the ranks' sum of the partials: LOSS_PARTIALS, LOSS_TAIL
enum { LOSS_WHOLE, LOSS_PARTIALS, LOSS_TAIL };
static int loss_forward(const mst_plan* p, int what, float* ws, const float* pitched, const float* unpitched, float* losses, hipStream_t st) {
    const mst_plan::LossOps& o = p->loss;
    const bool U = p->d.has_unpitched != 0;
    const float *pp = ws + o.pp, *up = U ? ws + o.up : nullptr, *ut = U ? unpitched : nullptr;
    float* scratch = ws + p->arena(SP_TMP) + p->loss_scratch;
    if (what == LOSS_PARTIALS) return loss_fwd_partials(pp, pitched, o.np, up, ut, o.nu, scratch, st);
    if (what == LOSS_TAIL)
        return loss_fwd_tail(o.np, o.nu, U ? 1 : 0, ws + o.il, ws + o.it, p->z.NI, ws + o.mlg, ws + o.mt, ws + o.bp, ws + o.bt, 1,
                             ws + o.losses, ws + o.saved, scratch, st, ws + o.gl, losses);
    return loss_fwd_batched(pp, pitched, o.np, up, ut, o.nu, ws + o.il, ws + o.it, p->z.NI, ws + o.mlg, ws + o.mt, ws + o.bp, ws + o.bt, 1,
                            ws + o.losses, ws + o.saved, scratch, p->loss_batch(), st, ws + o.gl, losses);
}
// pitched_grad: dL/d pitched_pred is written too; info_scale: see loss_bwd_batched
static int loss_backward(const mst_plan* p, float* ws, const float* pitched, const float* unpitched, bool pitched_grad, const LossBatch& lb,
                         float info_scale, hipStream_t st) {
    const mst_plan::LossOps& o = p->loss;
    const bool U = p->d.has_unpitched != 0;
    float* g = ws + p->arena(SP_GRAD);
    return loss_bwd_batched(ws + o.pp, pitched, o.np, U ? ws + o.up : nullptr, U ? unpitched : nullptr, o.nu, ws + o.il, ws + o.it, p->z.NI,
                            ws + o.mlg, ws + o.mt, ws + o.bp, ws + o.bt, ws + o.saved, ws + o.gl, pitched_grad ? g + o.pp : nullptr,
                            U ? g + o.up : nullptr, g + o.il, g + o.mlg, g + o.bp, lb, st, info_scale);
}

extern "C" int32_t mst_train_iteration(const mst_plan* p, const float* params, float* gparams, float* ws,
                                       const float* pitched, const float* unpitched, float* losses, mst_stream stream) {
    if (!p || !params || !gparams || !ws || !pitched) return MST_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    // the zero list (with the exchange tags) rides on the first forward launch where the plan proved that launch independent of it
    int e = p->zero_ride >= 0 ? 0 : mst_zero_grads(p, MST_STAGE_ALL, ws, stream);
    if (e) return e;
    if (p->d.has_unpitched && !unpitched) return MST_ERR_ARG;
    e = run_pass(p, p->list(MST_STAGE_ALL, 0), MST_STAGE_ALL, make_bases(p, params, nullptr, ws, pitched, unpitched), st, p->tags_in_zero, p->zero_ride);
    if (e) return e;
    e = loss_forward(p, LOSS_WHOLE, ws, pitched, unpitched, losses, st);
    if (e) return e;
    e = loss_backward(p, ws, pitched, unpitched, false /* the applier's backward kernel derives dL/d pitched_pred itself */, p->loss_batch(), 1.f, st);
    if (e) return e;
    e = backward_impl(p, MST_STAGE_ALL, params, gparams, ws, pitched, unpitched, stream, MST_BF_LOSS_FUSED);
    if (e) return e;
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------ evaluation
// mst_train_iteration without its backward half, plus the note metrics.  There is no zero launch here, so the forward runs as
// mst_forward runs it: the multi-workgroup LSTM's transpose step clears the exchange tags itself.
static int64_t eval_slices(const mst_plan* p, bool pitched) {
    return mst_roll_slices(pitched ? (int64_t)p->Q() * NF * NPN : (int64_t)p->Q() * NF * NUN);
}

extern "C" int64_t mst_eval_scratch_bytes(const mst_plan* p) {
    if (!p) return MST_ERR_ARG;
    if (p->tiled()) return MST_ERR_UNSUPPORTED;
    return 32 * (int64_t)p->K() * ((int64_t)p->d.C * eval_slices(p, true) + (p->d.has_unpitched ? eval_slices(p, false) : 0));
}

extern "C" int32_t mst_eval_iteration(const mst_plan* p, const float* params, float* ws, const float* pitched,
                                      const float* unpitched, float* losses, double* metrics, void* scratch, mst_stream stream) {
    if (!p || !params || !ws || !pitched || !metrics || !scratch || ((uintptr_t)metrics & 7) || ((uintptr_t)scratch & 7)) return MST_ERR_ARG;
    if (p->tiled()) return MST_ERR_UNSUPPORTED;
    if (p->d.has_unpitched && !unpitched) return MST_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    int e = run_pass(p, p->list(MST_STAGE_ALL, 0), MST_STAGE_ALL, make_bases(p, params, nullptr, ws, pitched, unpitched), st);
    if (e) return e;
    const bool U = p->d.has_unpitched != 0;
    const int K = p->K(), C = p->d.C;
    const mst_plan::LossOps& o = p->loss;
    e = loss_forward(p, LOSS_WHOLE, ws, pitched, unpitched, losses, st);
    if (e) return e;
    EvalMetricsArgs a{};
    a.part_p = scratch; a.slices_p = eval_slices(p, true); a.cells_p = o.np / C;
    e = launch_roll_metrics(ws + o.pp, pitched, (int64_t)K * C, a.cells_p, NPF, C, p->act_top, p->ext0_stride(), scratch, st);
    if (e) return e;
    if (U) {
        void* su = (char*)scratch + 32 * (int64_t)K * C * a.slices_p;
        a.part_u = su; a.slices_u = eval_slices(p, false); a.cells_u = o.nu;
        e = launch_roll_metrics(ws + o.up, unpitched, K, o.nu, NUF, 1, p->act_top, p->ext1_stride(), su, st);
        if (e) return e;
    }
    a.C = C; a.ni = p->z.NI;
    a.il = ws + o.il; a.it = ws + o.it; a.mlg = ws + o.mlg; a.mt = ws + o.mt;
    a.bp = ws + o.bp; a.bt = ws + o.bt; a.ws_stride = p->act_top; a.out = metrics;
    return launch_eval_metrics_finish(a, K, st);
}


// ------------------------------------------------------------------------------------------ tiled plans
// One train iteration (train-model.py:113-126) of ONE long clip whose bars are tiled over several ranks (BASELINE.json
// configs[4]).  Every rank builds a plan for its bar tile (mst_plan_options.tile_r0 / tile_rows) and walks the
// same phase list; after a phase that reports xlen > 0 the host all-reduces (SUM) ws[xoff, xoff + xlen) over the ranks
// before the next phase.  What crosses ranks: the last-beat states feeding the replicated bar-level LSTMs (an all-gather as a
// SUM over zero-padded buffers), the partial sums of every global reduction (combine's per-channel sums of squares and its
// backward's sum(g x), sum(g out); the loss sums) and, backward, the gradients of the gathered rows.  Everything else is local
// or replicated; gradients of replicated operations computed from a rank's PARTIAL upstream gradient add up to the true
// gradient in the final all-reduce of gparams because backward is linear in the upstream gradient — the song-info loss
// gradients, which are complete on every rank, are therefore seeded on the root rank only.
extern "C" int32_t mst_tiled_phase_count(const mst_plan* p) { return p ? (int32_t)p->phases.size() : MST_ERR_ARG; }

extern "C" int32_t mst_tiled_phase(const mst_plan* p, int32_t phase, const float* params, float* gparams, float* ws,
                                   const float* pitched, const float* unpitched, float* losses, int32_t is_root,
                                   mst_stream stream, int64_t* xoff, int64_t* xlen, int32_t* nx) {
    if (!p || !p->tiled() || phase < 0 || phase >= (int)p->phases.size() || !params || !gparams || !ws || !pitched || !xoff || !xlen || !nx)
        return MST_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    const mst_plan::Phase& ph = p->phases[phase];
    Bases b = make_bases(p, params, gparams, ws, pitched, unpitched);
    b.flags |= MST_BF_ALL_STAGES;
    const bool U = p->d.has_unpitched != 0;
    if (phase == 0) {
        if (launch_zero(p->d_zero_all, (int)p->zero_all.size(), 1, ws + p->arena(SP_GRAD), p->act_top, st)) return MST_ERR_LAUNCH;
        if (launch_zero(p->d_zero_fwd, (int)p->zero_fwd.size(), 1, ws, p->act_top, st)) return MST_ERR_LAUNCH;
    }
    if (ph.what == 0) {
        const std::vector<Step>& L = p->sched_all[ph.pass];
        for (int i = ph.begin; i < ph.end; ++i) {
            if (L[i].kind == K_XCHG) continue;          // an earlier exchange of the level this phase ends at: delivered with the others
            int e = run_step(p, L, L[i], b, st);
            if (e) return e < 0 ? e : MST_ERR_LAUNCH;
        }
        if (ph.pass == 1 && phase == (int)p->phases.size() - 1)
            for (int s = 2; s >= 0; --s)
                if (launch_slab_reduce(p->d_slabs[s], p->d_slab_blocks[s], (int)p->slab_blocks[s].size(), b, st)) return MST_ERR_LAUNCH;
    } else if (ph.what == 1) {
        int e = loss_forward(p, LOSS_PARTIALS, ws, pitched, unpitched, losses, st);
        if (e) return e;
        if (launch_fold(p->folds.dev + p->loss_fold[0], 0, b, st) || (U && launch_fold(p->folds.dev + p->loss_fold[1], 0, b, st))) return MST_ERR_LAUNCH;
    } else {
        if (launch_fold(p->folds.dev + p->loss_fold[0], 1, b, st) || (U && launch_fold(p->folds.dev + p->loss_fold[1], 1, b, st))) return MST_ERR_LAUNCH;
        int e = loss_forward(p, LOSS_TAIL, ws, pitched, unpitched, losses, st);
        if (e) return e;
        e = loss_backward(p, ws, pitched, unpitched, true, LossBatch{1, 0, 0, 0, 0, 0}, is_root ? 1.f : 0.f, st);
        if (e) return e;
    }
    *nx = ph.nx;
    for (int q = 0; q < ph.nx; ++q) {
        const mst_plan::Xchg& x = p->xchgs[ph.xchg[q]];
        xoff[q] = p->arena(x.space) + x.off; xlen[q] = x.len;
    }
    return hipGetLastError() == hipSuccess ? MST_OK : MST_ERR_LAUNCH;
}

// ------------------------------------------------------------------------------------------ instrumentation
// Per-launch-step timing with HIP events recorded on the caller's stream (bench.py's roofline leg).
// Not graph-capturable (it synchronises on events) and never called from the training path.
static void step_cost(const mst_plan* p, const Step& s, double* flops, double* bytes) {
    double f = 0, b = 0;
    switch (s.kind) {
    case K_GEMM: case K_GEMM_FOLD:
        for (int i = 0; i < s.count; ++i) {
            const GemmDesc& g = p->gemms.sched[s.first + i];
            f += 2.0 * g.M * g.N * g.K;
            b += 4.0 * ((double)g.M * g.K + (double)g.K * g.N + (double)g.M * g.N);
        }
        break;
    case K_GATHER:
        for (int i = 0; i < s.count; ++i) { const GatherDesc& g = p->gathers.sched[s.first + i]; b += 8.0 * g.rows * g.K; }
        break;
    case K_LIN_F: case K_LIN_A: case K_LIN_W: {
        const LinDesc& l = p->lins.host[s.first];
        const double rows = (double)l.clips * l.rows;
        f = 2.0 * rows * l.N * l.K;
        b = 4.0 * (rows * l.K + rows * l.N * (s.kind == K_LIN_F ? 1.0 : 2.0) + (double)l.N * l.K);
        break;
    }
    case K_CONV_F: case K_CONV_W: {
        const ConvDesc& c = p->convs.host[s.first];
        const double rows = (double)c.clips * c.P * NOCT, kk = NF * NPF * CONV_K;
        f = 2.0 * rows * c.OC * kk;
        b = 4.0 * (rows / NOCT * NF * NPN * NPF + rows * c.OC * (s.kind == K_CONV_F ? 1.0 : 2.0) + c.OC * kk);
        break;
    }
    case K_SEGRED:
        for (int i = 0; i < s.count; ++i) {
            const SegRedDesc& r = p->segreds.sched[s.first + i];
            const double rows = (double)r.d[0] * r.d[1] * r.d[2] * r.d[3];
            f += rows * r.width; b += 4.0 * (rows * r.width + 2.0 * r.nidx * r.width);
        }
        break;
    case K_LSTM_F: case K_LSTM_B:
        for (int i = 0; i < s.count; ++i) {
            const LstmDesc& l = p->lstms.sched[s.first + i];
            f += (double)l.B * l.S * (8.0 * l.H * l.H + 30.0 * l.H);
            b += 4.0 * ((double)l.B * l.S * 11.0 * l.H + 4.0 * l.H * l.H);
        }
        break;
    case K_COMB_F: case K_COMB_B:
        for (int i = 0; i < s.count; ++i) {
            const CombineDesc& c = p->combines.sched[s.first + i];
            const double n = (double)c.rows * c.cols;
            f += n * c.Cn * (s.kind == K_COMB_F ? 4.0 : 8.0);
            b += 4.0 * n * (s.kind == K_COMB_F ? 2.0 * c.Cn + 1 : 4.0 * c.Cn + 2);
        }
        break;
    case K_ROW_F: case K_ROW_B:
        for (int i = 0; i < s.count; ++i) {
            const RowLinDesc& r = p->rowlins.sched[s.first + i];
            const double mm = 2.0 * r.rows * r.kin * r.nout;
            f += s.kind == K_ROW_F ? mm : 2.0 * mm;
            b += 4.0 * r.rows * (s.kind == K_ROW_F ? r.kin + r.nout : 2.0 * r.kin + 2.0 * r.nout + (r.xgrad ? r.kin : 0));
        }
        break;
    case K_ME_SQ: case K_ME_F: case K_ME_RED: case K_ME_B: {
        // algorithmic = the reference's (unfused) shapes; the recomputation the fused kernels do on top is not counted
        const NotesDesc& n = p->notes.sched[s.first];
        const double pos = (double)n.C * n.Q * NF * NPN * s.count, mel = pos / n.C * n.W;
        const double per = 2.0 * n.W + 2.0 * n.CW * NPF + 2.0 * n.W * (n.W + n.CW);
        if (s.kind == K_ME_SQ) { f = pos * (per + 2.0 * n.W); b = 4.0 * pos * NPF; }
        else if (s.kind == K_ME_F) { f = pos * 2.0 * n.W; b = 4.0 * (pos * NPF + mel); }
        else if (s.kind == K_ME_RED) { f = pos * 2.0 * n.W; b = 4.0 * (pos * NPF + 2.0 * mel); }
        else { f = pos * per * 2.0; b = 4.0 * (pos * NPF + mel); }
        break;
    }
    case K_PSA_F: case K_PSA_B: {
        const NotesDesc& n = p->notes.sched[s.first];
        const double pos = (double)n.C * n.Q * NF * NPN * s.count;
        const double per = 2.0 * 30 + 2.0 * NPF * (30 + n.ML);
        f = pos * per * (s.kind == K_PSA_F ? 1.0 : 3.0);
        b = 4.0 * (pos * NPF * (s.kind == K_PSA_F ? 1.0 : 2.0) + (double)s.count * n.C * n.Q * NF * 450 * (s.kind == K_PSA_F ? 1.0 : 2.0) +
                   (double)s.count * n.Q * NF * NPN * n.ML * (s.kind == K_PSA_F ? 1.0 : 2.0));
        break;
    }
    }
    *flops = f; *bytes = b;
}

extern "C" int64_t mst_plan_zero_floats(const mst_plan* p, int32_t mask) {
    if (!p) return MST_ERR_ARG;
    int64_t n = 0;
    if ((mask & MST_STAGE_ALL) == MST_STAGE_ALL) { for (auto& c : p->zero_all) n += c.len; return n; }
    for (int s = 0; s < 3; ++s) if ((mask >> s) & 1) for (auto& c : p->zero_stage[s]) n += c.len;
    return n;
}

extern "C" int32_t mst_plan_step_carried(const mst_plan* p, int32_t mask, int32_t backward, int32_t* carried) {
    if (!p || !carried) return MST_ERR_ARG;
    int n = 0;
    for (const Step* s : steps_of(p, mask, backward))
        carried[n++] = (s->carrier < 0 || (s->kind != K_GATHER && s->kind != K_SEGRED)) ? 0 : (second_stage(*s) ? 2 : 1);
    return n;
}

// every kind: 0 = own launch(es), 1 = the whole step is in its level's GEMM launch, 2 = the first stage is carried and the second
// stage is a launch behind the carrier
extern "C" int32_t mst_plan_step_riders(const mst_plan* p, int32_t mask, int32_t backward, int32_t* out) {
    if (!p || !out) return MST_ERR_ARG;
    int n = 0;
    for (const Step* s : steps_of(p, mask, backward))
        out[n++] = (s->carrier < 0 || s->kind == K_LSTM_F || s->kind == K_LSTM_B) ? 0 : (second_stage(*s) ? 2 : 1);      // LSTM steps: mst_plan_step_carrier
    return n;
}

// for every step of the list: the index, within the same (mask-filtered) list, of the step whose launch runs it; -1 = its own launch
extern "C" int32_t mst_plan_step_carrier(const mst_plan* p, int32_t mask, int32_t backward, int32_t* out) {
    if (!p || !out) return MST_ERR_ARG;
    const std::vector<Step>& L = p->list(mask, backward);
    const std::vector<const Step*> steps = steps_of(p, mask, backward);
    std::vector<int> pos(L.size(), -1);             // list index -> index among the steps of `mask`
    int n = 0;
    for (const Step* s : steps) pos[s - L.data()] = n++;
    for (const Step* s : steps) *out++ = s->carrier < 0 ? -1 : pos[s->carrier];
    return n;
}

// on = 0: the plan's own-launch H <= 16 LSTM steps use the register-flavour kernels instead of the one-wave ones (tests, profiling)
extern "C" int32_t mst_plan_set_lstm_small(mst_plan* p, int32_t on) {
    if (!p) return MST_ERR_ARG;
    for (int pass = 0; pass < 2; ++pass)
        for (const std::vector<Step>* L : {&p->sched[pass], &p->sched_all[pass]})
            for (const Step& s : *L)
                if ((s.kind == K_LSTM_F || s.kind == K_LSTM_B) && s.carrier >= 0) return MST_ERR_UNSUPPORTED;      // run inside a gemm_kernel launch
    p->lstm_small_on = on ? 1 : 0;          // read by run_step at each launch
    return MST_OK;
}

extern "C" int32_t mst_plan_zero_rides(const mst_plan* p) { return !p ? MST_ERR_ARG : (p->zero_ride >= 0 ? 1 : 0); }

extern "C" int32_t mst_plan_step_count(const mst_plan* p, int32_t mask, int32_t backward) {
    return p ? (int32_t)steps_of(p, mask, backward).size() : MST_ERR_ARG;
}

// shape of step i of a pass: GEMM {M,N,K,ksplit} of its first descriptor (+count), LSTM {B,S,H,count},
// segment-reduce {nidx max, width, rows, count}; then the member count, the step kind, its dependency level and its chain (-1: none)
extern "C" int32_t mst_plan_step_info(const mst_plan* p, int32_t mask, int32_t backward, int32_t* info /* 8 per step */) {
    if (!p || !info) return MST_ERR_ARG;
    int idx = 0;
    for (const Step* s : steps_of(p, mask, backward)) {
        int32_t* o = info + 8 * idx++;
        o[0] = o[1] = o[2] = o[3] = 0; o[4] = s->count; o[5] = s->kind; o[6] = s->lvl; o[7] = s->chain;
        if (s->kind == K_GEMM || s->kind == K_GEMM_FOLD) { const GemmDesc& g = p->gemms.sched[s->first]; o[0] = g.M; o[1] = g.N; o[2] = g.K; o[3] = g.ksplit; }
        else if (KINDS[s->kind].fam == F_LIN) { const LinDesc& l = p->lins.host[s->first]; o[0] = l.rows; o[1] = l.N; o[2] = l.K; o[3] = l.splits; }
        else if (s->kind == K_LSTM_F || s->kind == K_LSTM_B) { const LstmDesc& l = p->lstms.sched[s->first]; o[0] = l.B; o[1] = l.S; o[2] = l.H; o[3] = l.multi; }
        else if (s->kind == K_GATHER) { const GatherDesc& g = p->gathers.sched[s->first]; o[0] = g.rows; o[1] = g.K; o[2] = g.nseg; }
        else if (s->kind == K_SEGRED) { const SegRedDesc& r = p->segreds.sched[s->first]; o[0] = s->a; o[1] = r.width; o[2] = r.d[0] * r.d[1] * r.d[2] * r.d[3]; }
        else if (s->kind == K_COMB_F || s->kind == K_COMB_B) { const CombineDesc& c = p->combines.sched[s->first]; o[0] = c.Cn; o[1] = c.rows; o[2] = c.cols; o[3] = c.nblk; }
    }
    return idx;
}

// members of GEMM step i of a pass, one clip's worth: {M, N, K, ksplit, fold_rows, workgroups} each (tools/step_profile.py)
extern "C" int32_t mst_plan_step_gemms(const mst_plan* p, int32_t mask, int32_t backward, int32_t step, int32_t* out, int32_t cap) {
    if (!p || !out) return MST_ERR_ARG;
    const std::vector<const Step*> steps = steps_of(p, mask, backward);
    if (step < 0 || step >= (int)steps.size()) return MST_ERR_ARG;
    const Step& s = *steps[step];
    if (s.kind != K_GEMM && s.kind != K_GEMM_FOLD) return 0;
    int n = 0;
    for (int q = 0; q < s.b && n < cap; ++q, ++n) {
        const GemmDesc& g = p->gemms.sched[s.first + q];
        int32_t* o = out + 6 * n;
        o[0] = g.M; o[1] = g.N; o[2] = g.K; o[3] = g.ksplit; o[4] = g.fold_rows; o[5] = gemm_blocks(g, p->mfma);
    }
    return n;
}

extern "C" int32_t mst_plan_step_gemm_kinds(const mst_plan* p, int32_t mask, int32_t backward, int32_t step, int32_t* out, int32_t cap) {
    if (!p || !out) return MST_ERR_ARG;
    const std::vector<const Step*> steps = steps_of(p, mask, backward);
    if (step < 0 || step >= (int)steps.size()) return MST_ERR_ARG;
    const Step& s = *steps[step];
    if (s.kind != K_GEMM && s.kind != K_GEMM_FOLD) return 0;
    int n = 0;
    for (int q = 0; q < s.b && n < cap; ++q, ++n) {
        const GemmDesc& g = p->gemms.sched[s.first + q];
        out[2 * n] = g.variant; out[2 * n + 1] = p->mfma ? 32 : 32 << g.kdsel;
    }
    return n;
}

extern "C" int32_t mst_plan_time_steps(const mst_plan* p, int32_t mask, int32_t backward, const float* params, float* gparams,
                                       float* ws, const float* pitched, const float* unpitched, mst_stream stream,
                                       int32_t reps, float* ms, int32_t* kind, double* flops, double* bytes) {
    if (!p || !params || !ws || !ms || !kind || !flops || !bytes || reps < 1) return MST_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    Bases b = make_bases(p, params, gparams, ws, pitched, unpitched);
    if (backward && !p->tiled()) b.flags = MST_BF_LOSS_FUSED;          // what mst_train_iteration launches
    if ((mask & MST_STAGE_ALL) == MST_STAGE_ALL) b.flags |= MST_BF_ALL_STAGES;
    hipEvent_t e0, e1;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return MST_ERR_ALLOC;
    const std::vector<Step>& L = p->list(mask, backward);
    int idx = 0;
    for (const Step* s : steps_of(p, mask, backward)) {
        float t = 0.f;
        if (s->carrier < 0) {                         // a carried step is timed inside its carrier's: 0 ms here, with its own work
            run_step(p, L, *s, b, st);                // warm
            hipEventRecord(e0, st);
            for (int r = 0; r < reps; ++r) run_step(p, L, *s, b, st);
            hipEventRecord(e1, st);
            hipEventSynchronize(e1);
            hipEventElapsedTime(&t, e0, e1);
        }
        ms[idx] = t / reps; kind[idx] = s->kind == K_GEMM_FOLD ? K_GEMM : s->kind;      // same kernel
        step_cost(p, *s, &flops[idx], &bytes[idx]);
        ++idx;
    }
    hipEventDestroy(e0); hipEventDestroy(e1);
    return idx;
}

extern "C" const char* mst_version(void) { return "mst_amd 0.1 (gfx950)"; }
