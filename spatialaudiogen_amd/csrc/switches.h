// Every environment switch of the native library, declared once (host-only: no HIP in here).  INTEGRATION.md 5 is written from this table.
// Code that has a context reads its copy, `c->sw`, made when the context is created (sagen_create_impl) - the rows that name an option are
// the ones sagen_set_option changes on that copy.  Code that has none (launchers, op level) reads process_switches(), made at first use.
#pragma once
#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>

namespace sagen {

// The kinds of row (tag: what tests/switches_listing.cpp prints).  "Set" means present in the environment, whatever the value: SAGEN_NO_H2=0 and an empty value switch too.
struct SwOn { using type = bool; static constexpr char tag = '+'; static bool read(const char* e, bool dflt) { return e ? true : dflt; } };        // a flag that is on when the variable is set
struct SwOff { using type = bool; static constexpr char tag = '-'; static bool read(const char* e, bool dflt) { return e ? false : dflt; } };      // a flag that is off when the variable is set
// atol of the value, clamped to LO..HI; the default (not clamped) when the variable is not set
template <long LO, long HI> struct SwInt { using type = long; static constexpr char tag = 'i'; static long read(const char* e, long dflt) { return !e ? dflt : std::min(HI, std::max(LO, atol(e))); } };
struct SwStr { using type = const char*; static constexpr char tag = 's'; static const char* read(const char* e, const char* dflt) { return e ? e : dflt; } };      // the value itself (the environment's own storage: sagen_create_impl reads it at once)
#define SW_INT(lo, hi) SwInt<lo, hi>
#define SW_ANY SwInt<LONG_MIN, LONG_MAX>
constexpr long SW_UNSET = LONG_MIN;             // default of an integer row whose site asks "was it given?"

// X(member, kind, default, environment name, sagen_set_option name or nullptr, doc)
#define SAGEN_SWITCHES(X) \
    /* numeric formats and plane-fed kernels */ X(fp32_only, SwOn, false, "SAGEN_FP32_ONLY", nullptr, "only the exact fp32 MFMA kernels: no bf16x3 / fp16x2 tiles, no planes (heuristics, tuner, weight gradients)") \
    X(no_p3, SwOn, false, "SAGEN_NO_P3", nullptr, "the stride-1 3x3 trunk convs never read pre-split planes (conv3p.hip / conv3h.hip)") \
    X(want_p3_from_stage, SW_ANY, SW_UNSET, "SAGEN_P3_FROM_STAGE", nullptr, "... from this ResNet stage on (2..5); not set: 2 with the fp16x2 planes, 3 with bf16 planes; per context \"planes_from_stage\"") \
    X(use_h2, SwOff, true, "SAGEN_NO_H2", "fp16x2", "the trunk's planes are two fp16 planes (conv3h.hip, three products per multiply); off: three bf16 planes (conv3p.hip, six products)") \
    X(p3g, SwOn, false, "SAGEN_P3G", nullptr, "conv3g_kernel for the stride-2 conv_1 + shortcut of stages 3-5 also on bf16 planes (default: with the fp16x2 planes only); per context \"plane_gather\"") \
    X(no_p3g, SwOn, false, "SAGEN_NO_P3G", nullptr, "... never") \
    X(use_s2d, SwOff, true, "SAGEN_NO_S2D", "plane_s2d", "lean trunk: a stage's last merge writes its planes in space-to-depth form for the next stage's stride-2 conv_1 (conv3s.hip); off: the gathered kernel everywhere") \
    X(no_lean_trunk, SwOn, false, "SAGEN_NO_LEAN_TRUNK", nullptr, "the ResNet merges read fp32 residuals and write fp32 block outputs next to the planes (round 4)") \
    X(no_aud_planes, SwOn, false, "SAGEN_NO_AUDIO_PLANES", nullptr, "conv2 .. conv5 of the audio encoder stay on the register-staged kernels instead of conv3g_kernel on fp16x2 planes (round 6)") \
    /* stems */ X(stem8, SwOff, true, "SAGEN_NO_STEM8", "u8_fast_stem", "uint8 frames run the one-operand-plane stem (stem8.hip); off: the general kernels, bit-identical to the float entry point") \
    X(stem8h, SwOff, true, "SAGEN_NO_STEM8_H2", "u8_stem_h2", "... one fp16 plane x two fp16 filter planes (MODE 2); off: the bf16 plane x three bf16 filter planes of round 4") \
    X(stem16, SwOff, true, "SAGEN_NO_STEM16", "f16_fast_stem", "float frames run the fp16x2 variant of that kernel (two planes scaled by the frame's exact maximum); off: igemm3s2_kernel + the pool pass") \
    X(no_stempool, SwOn, false, "SAGEN_NO_STEMPOOL", nullptr, "never the fused stem + max-pool kernel (stempool.hip)") \
    X(stempool, SwOn, false, "SAGEN_STEMPOOL", nullptr, "... also under SAGEN_ONE_STREAM") \
    /* streams */ X(one_stream, SwOn, false, "SAGEN_ONE_STREAM", nullptr, "a context never uses its own second stream (a host that keeps several batches in flight, DESIGN.md 6.1)") \
    X(no_fork2, SwOn, false, "SAGEN_NO_FORK2", nullptr, "no second fork: the localisation FCs stay on the caller's stream next to the mask decoder") \
    X(aux_prio, SwStr, nullptr, "SAGEN_AUX_PRIO", nullptr, "low|high: the second stream below / above the default priority (experiment, measured harmful: DESIGN.md 6.1)") \
    /* FC layers, split-K, tuner */ X(fcm, SwOn, false, "SAGEN_FCM", nullptr, "the skinny FC layers run fcm_kernel (fcm.hip) chained through partials - measured slower (DESIGN.md 3.2)") \
    X(sk_fused, SwOn, false, "SAGEN_SK_FUSED", nullptr, "split-K partials are combined inside the contraction (last arriver) instead of by a reducer launch - bit-identical, measured no faster (DESIGN.md 7)") \
    X(no_autotune, SwOn, false, "SAGEN_NO_AUTOTUNE", nullptr, "sagen_autotune / sagen_train_autotune return at once (the shape heuristics stay in force)") \
    X(no_dh_split, SwOn, false, "SAGEN_NO_DH_SPLIT", nullptr, "the tuner does not consider conv3h_kernel's dh-split (one filter row per workgroup, round 6)") \
    X(p3pp, SwOn, false, "SAGEN_P3PP", nullptr, "the tuner considers conv3pp_kernel (two teams, 121 KiB of LDS) at inference too") \
    X(p3hr, SwOn, false, "SAGEN_P3HR", nullptr, "the tuner considers conv3hr_kernel (three-deep activation ring) for ungrouped contexts too") \
    X(tune_groups, SW_ANY, 0, "SAGEN_TUNE_GROUPS", nullptr, "groups a tuning pass launches per candidate (0 = all: tuned on 4 of 15 groups 1 % slower in 10 s instead of 14 s)") \
    X(force_tile, SW_ANY, SW_UNSET, "SAGEN_FORCE_TILE", nullptr, "tuning knob of the op-level heuristics: this IgemmTile index wherever it can run") \
    /* mask decoder */ X(no_scatter, SwOn, false, "SAGEN_NO_DECONV_SCATTER", nullptr, "deconv5 .. deconv2 as depth-to-space convs over the full output grid (round 4): no scatter form, no live-row bands") \
    X(no_decoder_planes, SwOn, false, "SAGEN_NO_DECODER_PLANES", nullptr, "the scatter form on the fp32 concat buffers instead of fp16x2 planes; per context \"decoder_planes\"") \
    X(no_d1_planes, SwOn, false, "SAGEN_NO_DECONV1_PLANES", nullptr, "deconv1 on igemm3_kernel instead of conv3g_kernel + planes of cat1") \
    X(no_maskfuse, SwOn, false, "SAGEN_NO_MASKFUSE", nullptr, "deconv1 and the mask application stay two kernels; per context \"materialize_mask\"") \
    /* training step */ X(train_h2, SwOff, true, "SAGEN_TRAIN_NO_H2", nullptr, "the training forward runs the trunk's stride-1 3x3 convs on the fp16x2 planes; off: bf16x3") \
    X(train_h2d, SwOff, true, "SAGEN_TRAIN_NO_H2D", nullptr, "... its backward runs their data gradients on fp16x2 planes of dy, written by the batch-norm backward; off: bf16x3 on fp32 dy") \
    X(train_h2w, SwOff, true, "SAGEN_TRAIN_NO_H2W", nullptr, "... and their weight gradients on the planes the forward retains (wgrad3h.hip); off: the fp32 tensors, nothing retained") \
    X(train_bands, SwOff, true, "SAGEN_TRAIN_NO_BANDS", "train_bands", "the training step's decoder on the live rows only, forward and backward; off: full tensors (round 4)") \
    X(train_rawpool, SwOff, true, "SAGEN_TRAIN_NO_RAWPOOL", "train_rawpool", "the training forward's stem writes the raw output and its pooled extremum; off: a pool pass of its own") \
    X(train_no_dec_planes, SwOn, false, "SAGEN_TRAIN_NO_DEC_PLANES", nullptr, "the training forward's decoder on the register-staged kernels (fp32 operands), as up to round 5") \
    X(train_keep_a1, SwOn, false, "SAGEN_TRAIN_KEEP_A1", nullptr, "A/B: the training forward also writes the fp32 copy of every conv_2 input although the planes are retained") \
    X(train_no_relu_bits, SwOn, false, "SAGEN_TRAIN_NO_RELU_BITS", nullptr, "A/B: conv_2's batch-norm backward reads the fp32 block output for its ReLU mask, not the one-bit mask") \
    X(bn_read_act, SwOn, false, "SAGEN_BN_READ_ACT", nullptr, "A/B: the batch-norm backward reads the retained activation for its sign") \
    X(stem_bwd_unfused, SwOn, false, "SAGEN_STEM_BWD_UNFUSED", nullptr, "A/B: the stem's pool + batch-norm backward as three kernels") \
    X(no_split_repack, SwOn, false, "SAGEN_NO_SPLIT_REPACK", nullptr, "A/B: all forward filter packs on the caller's stream before the forward") \
    X(dgrad_packs_first, SwOn, false, "SAGEN_DGRAD_PACKS_FIRST", nullptr, "A/B: the data-gradient packs in front of the forward's second-stream work (the round-3 order)") \
    X(bwd_one_stream, SwOn, false, "SAGEN_BWD_ONE_STREAM", nullptr, "the weight gradients and the data-gradient packs stay on the caller's stream") \
    X(bwd_nosplit, SwOn, false, "SAGEN_BWD_NOSPLIT", nullptr, "debugging: no split-K in the data-gradient contractions") \
    /* launchers and packs of the training step (no context: process_switches()) */ X(wgrad_f32, SwOn, false, "SAGEN_WGRAD_F32", nullptr, "weight gradients on the exact fp32 MFMA kernel instead of bf16x3 (SAGEN_FP32_ONLY implies it)") \
    X(wgrad_ref, SwOn, false, "SAGEN_WGRAD_REF", nullptr, "weight gradients through the one-thread-per-element fp64 reference kernel") \
    X(wgrad_norow, SwOn, false, "SAGEN_WGRAD_NOROW", nullptr, "A/B: per-tap instead of filter-row weight gradients (and none on planes)") \
    X(wgrad_no_h2, SwOn, false, "SAGEN_WGRAD_NO_H2", nullptr, "A/B: weight gradients never on fp16x2 planes (the forward still retains them)") \
    X(wgrad_nofold, SwOn, false, "SAGEN_WGRAD_NOFOLD", nullptr, "A/B: no row folding for the stem / audio conv1 weight gradients") \
    X(wgrad_wgs, SW_INT(64, LONG_MAX), 0, "SAGEN_WGRAD_WGS", nullptr, "A/B: split-K workgroup target of the weight gradients (0 = 512 or 1024 by partial-sum traffic)") \
    X(dgrad_unphased, SwOn, false, "SAGEN_DGRAD_UNPHASED", nullptr, "the stride-2 data gradients as one padded contraction instead of one per output phase") \
    X(dgrad_phase_tiles, SW_ANY, 512, "SAGEN_DGRAD_PHASE_TILES", nullptr, "... the 3x3 ones go phase-wise from this many 64x64 tiles per phase on (tests: 0 = always)") \
    X(bwd_amort, SW_INT(1, LONG_MAX), 4, "SAGEN_BWD_AMORT", nullptr, "items per thread of the elementwise backward passes (1 = the round-4 grids)") \
    X(p3_amort, SW_ANY, 0, "SAGEN_P3_AMORT", nullptr, "items per thread of the plane passes (0 or less = 4)") \
    X(red_blocks, SW_INT(64, 1024), 512, "SAGEN_RED_BLOCKS", nullptr, "A/B: workgroups of the per-channel reductions (512 = two per CU)") \
    X(poolbwd_grid, SW_ANY, 2048, "SAGEN_POOLBWD_GRID", nullptr, "A/B: largest grid of the max-pool backward's gather pass") \
    X(relu_bwd_two_launches, SwOn, false, "SAGEN_RELU_BWD_TWO_LAUNCHES", nullptr, "A/B: small ReLU backward + column sum as two launches")

struct Switches {                               // constructing one reads the environment
#define X(member, kind, dflt, env, opt, doc) kind::type member = kind::read(getenv(env), dflt);
    SAGEN_SWITCHES(X)
#undef X
};
inline Switches read_switches() { return Switches(); }                                                  // a fresh read
inline const Switches& process_switches() { static const Switches s = read_switches(); return s; }      // read once per process, at first use
// sagen_set_option: sets the flag of the row that names option `name`
inline bool sw_set(bool& flag, const char* opt, const char* name, int value) { if (!opt || strcmp(opt, name) != 0) return false; flag = value != 0; return true; }
template <class T> bool sw_set(T&, const char*, const char*, int) { return false; }

}  // namespace sagen
