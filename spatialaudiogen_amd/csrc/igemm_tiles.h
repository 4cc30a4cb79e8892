// The registry of the contraction tiles: one row X(id, family, (template arguments)[, bm, bn, bk]) per instantiation of the IgemmDesc kernel
// families, each fact spelled ONCE.  enum IgemmTile (kernels.h), the tile table (igemm.hip: name, traits, shape) and the `case` lines of every
// *_dispatch are generated from the rows.  A row's index is the tile id of plans and tools: new rows go at the END.  No blanks in the arguments.
#pragma once

#define SAGEN_TILES(X) \
    /* exact fp32 MFMA (igemm_kernel<BM,BN,WM,WN,STAGES,BK>).  The first six are the shape-heuristic set; the rest exist for the autotuner (2-stage LDS ring = less LDS, more resident workgroups; extra aspect ratios) */ \
    X(128x128,             F32,     (128,128,64,64,3,16)) \
    X(128x64,              F32,     (128,64,64,32,3,16)) \
    X(256x64,              F32,     (256,64,64,64,3,16)) \
    X(64x64,               F32,     (64,64,32,32,3,16)) \
    X(128x32,              F32,     (128,32,32,32,2,16)) \
    X(32x128,              F32,     (32,128,32,32,2,16)) \
    X(128x128_S2,          F32,     (128,128,64,64,2,16)) \
    X(128x64_S2,           F32,     (128,64,64,32,2,16)) \
    X(256x64_S2,           F32,     (256,64,64,64,2,16)) \
    X(64x64_S2,            F32,     (64,64,32,32,2,16)) \
    X(64x128,              F32,     (64,128,32,64,3,16)) \
    X(64x128_S2,           F32,     (64,128,32,64,2,16)) \
    X(64x256,              F32,     (64,256,64,64,3,16)) \
    X(64x256_S2,           F32,     (64,256,64,64,2,16)) \
    X(256x32,              F32,     (256,32,64,32,2,16)) \
    /* ... K tile of 32 (half the barriers per MFMA; needs Kpad % 32 == 0) */ \
    X(64x64_K32,           F32,     (64,64,32,32,2,32)) \
    X(64x128_K32,          F32,     (64,128,32,64,2,32)) \
    X(128x64_K32,          F32,     (128,64,64,32,2,32)) \
    X(128x128_K32,         F32,     (128,128,64,64,2,32)) \
    X(32x128_K32,          F32,     (32,128,32,32,2,32)) \
    X(128x32_K32,          F32,     (128,32,32,32,2,32)) \
    /* fp32-equivalent bf16x3 operand split on the bf16 matrix cores (igemm3_kernel<BM,BN,WM,WN,KS>; needs IgemmDesc::w_split); KS = 2: two K tiles of 16 per barrier step */ \
    X(B3_128x128,          B3,      (128,128,64,64,1)) \
    X(B3_128x64,           B3,      (128,64,64,32,1)) \
    X(B3_256x64,           B3,      (256,64,64,64,1)) \
    X(B3_64x64,            B3,      (64,64,32,32,1)) \
    X(B3_64x128,           B3,      (64,128,32,64,1)) \
    X(B3_64x256,           B3,      (64,256,64,64,1)) \
    X(B3_32x128,           B3,      (32,128,32,32,1)) \
    X(B3_128x32,           B3,      (128,32,32,32,1)) \
    X(B3_128x64_K2,        B3,      (128,64,64,32,2)) \
    X(B3_64x64_K2,         B3,      (64,64,32,32,2)) \
    X(B3_64x128_K2,        B3,      (64,128,32,64,2)) \
    X(B3_32x128_K2,        B3,      (32,128,32,32,2)) \
    X(B3_128x32_K2,        B3,      (128,32,32,32,2)) \
    /* bf16x3 for dense 3x3 stride-1 SAME convs: the three horizontal taps share one activation tile (igemm3dw_kernel<BM,BN,WM,WN,MERGE>); MERGE: the three taps also share one barrier step (narrow N) */ \
    X(B3DW_128x128,        B3DW,    (128,128,64,64,false)) \
    X(B3DW_128x64,         B3DW,    (128,64,64,32,false)) \
    X(B3DW_256x64,         B3DW,    (256,64,64,64,false)) \
    X(B3DW_64x128,         B3DW,    (64,128,32,64,false)) \
    X(B3DW_64x64,          B3DW,    (64,64,32,32,false)) \
    X(B3DW_64x256,         B3DW,    (64,256,64,64,false)) \
    X(B3DWM_128x64,        B3DW,    (128,64,64,32,true)) \
    X(B3DWM_256x64,        B3DW,    (256,64,64,64,true)) \
    X(B3DWM_64x64,         B3DW,    (64,64,32,32,true)) \
    X(B3DWM_64x128,        B3DW,    (64,128,32,64,true)) \
    /* bf16x3 for the 7x7 stride-2 stem over the padded 4-channel image, K ordered (dh, dw padded to 8, c) (igemm3s2_kernel<BM,BN,WM,WN>) */ \
    X(B3S2_256x64,         B3S2,    (256,64,64,64)) \
    X(B3S2_128x64,         B3S2,    (128,64,64,32)) \
    /* bf16x3 for dense 3x3 stride-1 SAME convs over pre-split activation planes (conv3p_kernel<BM,BN,WM,WN>; needs IgemmDesc::xp3) */ \
    X(P3_128x64,           P3,      (128,64,64,32)) \
    X(P3_128x128,          P3,      (128,128,64,64)) \
    X(P3_64x64,            P3,      (64,64,32,32)) \
    /* ... two phase-locked 4-wave teams per workgroup (conv3pp_kernel<MODE>): two 128x64 tiles / the two K halves of one */ \
    X(P3PP_PAIR,           P3PP,    (0), 128, 64, 16) \
    X(P3PP_SPLITK,         P3PP,    (1), 128, 64, 16) \
    /* bf16x3 for ANY strided / multi-tap conv over pre-split activation planes, operand tiles gathered by LDS-DMA (conv3g_kernel<BM,BN,WM,WN,KS,H2[,EPI]>) */ \
    X(P3G_128x64_K2,       P3G,     (128,64,64,32,2)) \
    X(P3G_64x64_K2,        P3G,     (64,64,32,32,2)) \
    X(P3G_64x128_K2,       P3G,     (64,128,32,64,2)) \
    X(P3G_128x128_K1,      P3G,     (128,128,64,64,1)) \
    /* fp16x2 for dense 3x3 stride-1 SAME convs over TWO fp16 planes per operand: three products per multiply (conv3h_kernel<BM,BN,WM,WN,KC>) */ \
    X(P3H_128x64,          P3H,     (128,64,64,32,1)) \
    X(P3H_128x128,         P3H,     (128,128,64,64,1)) \
    X(P3H_64x64,           P3H,     (64,64,32,32,1)) \
    X(P3H_256x64,          P3H,     (256,64,64,64,1)) \
    /* ... and for any strided / multi-tap conv over them (conv3g_kernel, gathered operand tiles) */ \
    X(P3GH_128x64_K3,      P3GH,    (128,64,64,32,3)) \
    X(P3GH_64x64_K4,       P3GH,    (64,64,32,32,4)) \
    X(P3GH_128x128_K2,     P3GH,    (128,128,64,64,2)) \
    X(P3GH_64x128_K3,      P3GH,    (64,128,32,64,3)) \
    /* conv3h_kernel with two / four 16-channel chunks per barrier step (the deep, latency-bound layers) */ \
    X(P3H_128x64_C2,       P3H,     (128,64,64,32,2)) \
    X(P3H_64x64_C2,        P3H,     (64,64,32,32,2)) \
    X(P3H_64x64_C4,        P3H,     (64,64,32,32,4)) \
    /* conv3g_kernel on fp16x2 planes with the fused decoder tail as its epilogue (deconv1 at inference: IgemmDesc::mm_out), 2 / 4 K tiles per group */ \
    X(P3GH_MM_64x128_K2,   P3GH_MM, (64,128,32,64,2)) \
    X(P3GH_MM_64x128_K4,   P3GH_MM, (64,128,32,64,4)) \
    X(P3GH_MM_128x128_K2,  P3GH_MM, (128,128,64,64,2)) \
    X(P3GH_MM_128x256_K2,  P3GH_MM, (128,256,64,128,2)) \
    /* conv3hr_kernel<BM,BN,WM,WN,KC>: conv3h_kernel with a three-deep ring of activation images beside the two filter stages (conv3h.hip); 128x128: 72 KB of LDS, two workgroups per CU */ \
    X(P3HR_256x64,         P3HR,    (256,64,64,64,1)) \
    X(P3HR_128x64,         P3HR,    (128,64,64,32,1)) \
    X(P3HR_64x64_C2,       P3HR,    (64,64,32,32,2)) \
    X(P3HR_128x128,        P3HR,    (128,128,64,64,1)) \
    /* the space-to-depth conv3h_kernel<BM,BN,WM,WN,KC,AR,true> (conv3s.hip): the 3x3 stride-2 SAME conv over space-to-depth fp16x2 planes (IgemmDesc::xs2d), conv3h_kernel's K loop; AR = depth of the activation ring (P3SR: three) */ \
    X(P3S_128x128,         P3S,     (128,128,64,64,1,2)) \
    X(P3SR_128x64,         P3S,     (128,64,64,32,1,3)) \
    X(P3SR_256x64,         P3S,     (256,64,64,64,1,3))

namespace sagen {
// What a kernel family is, by name (every tile of a family shares it).  Operand format: exact fp32 MFMA unless TF_BF16X3 / TF_FP16X2.
enum TileTrait : unsigned {
    TF_BF16X3 = 1,          // the bf16x3 operand split (needs IgemmDesc::w_split)
    TF_FP16X2 = 2,          // two fp16 planes per operand (needs w_split and IgemmDesc::wh2)
    TF_PLANES = 4,          // fed by pre-split activation planes (IgemmDesc::xp3 / xs2d), not by the fp32 tensor
    TF_GATHERED = 8,        // conv3g_kernel: operand tiles gathered by LDS-DMA - any stride / tap set on the plane rows
    TF_SHARED_TAPS = 16,    // dense 3x3 stride-1 SAME conv whose three horizontal taps share one activation tile
    TF_STEM = 32,           // igemm3s2_kernel: the 7x7 stride-2 stem
    TF_S2D = 64,            // the space-to-depth conv3h_kernel (contracts IgemmDesc::xs2d)
    TF_RING3 = 128,         // conv3hr_kernel: the three-deep activation ring as a kernel of its own
    TF_FUSED_TAIL = 256,    // the fused decoder tail is the epilogue (IgemmDesc::mm_out)
    TF_TWO_TEAM = 512,      // conv3pp_kernel: two phase-locked 4-wave teams per workgroup
    TF_GROUPED = 1024,      // takes the group index of a grouped launch from its grid (common.h: GroupInfo)
    TF_DH_SPLIT = 2048,     // can split K by the filter row (split-K = 3 exactly, one filter row per workgroup)
};
}  // namespace sagen

// One line per family: USE(id, the instantiation name as rocprofv3 prints it, the traits, the launch the dispatcher instantiates)
#define SAGEN_TILE_STR(...) #__VA_ARGS__
#define SAGEN_TILE_FAM_F32(USE, id, ...)     USE(id, "igemm_kernel<" SAGEN_TILE_STR(__VA_ARGS__) ">", TF_GROUPED, launch_cfg<__VA_ARGS__>)
#define SAGEN_TILE_FAM_B3(USE, id, ...)      USE(id, "igemm3_kernel<" SAGEN_TILE_STR(__VA_ARGS__) ">", TF_BF16X3 | TF_GROUPED, launch_cfg3<__VA_ARGS__>)
#define SAGEN_TILE_FAM_B3DW(USE, id, ...)    USE(id, "igemm3dw_kernel<" SAGEN_TILE_STR(__VA_ARGS__) ">", TF_BF16X3 | TF_SHARED_TAPS, launch_cfg3dw<__VA_ARGS__>)
#define SAGEN_TILE_FAM_B3S2(USE, id, ...)    USE(id, "igemm3s2_kernel<" SAGEN_TILE_STR(__VA_ARGS__) ">", TF_BF16X3 | TF_STEM, launch_cfg3s2<__VA_ARGS__>)
#define SAGEN_TILE_FAM_P3(USE, id, ...)      USE(id, "conv3p_kernel<" SAGEN_TILE_STR(__VA_ARGS__) ">", TF_BF16X3 | TF_PLANES | TF_SHARED_TAPS, launch_conv3p<__VA_ARGS__>)
#define SAGEN_TILE_FAM_P3PP(USE, id, ...)    USE(id, "conv3pp_kernel<" SAGEN_TILE_STR(__VA_ARGS__) ">", TF_BF16X3 | TF_PLANES | TF_SHARED_TAPS | TF_TWO_TEAM, launch_conv3pp<__VA_ARGS__>)
#define SAGEN_TILE_FAM_P3G(USE, id, ...)     USE(id, "conv3g_kernel<" SAGEN_TILE_STR(__VA_ARGS__) ",false>", TF_BF16X3 | TF_PLANES | TF_GATHERED | TF_GROUPED, launch_conv3g<__VA_ARGS__, false>)
#define SAGEN_TILE_FAM_P3GH(USE, id, ...)    USE(id, "conv3g_kernel<" SAGEN_TILE_STR(__VA_ARGS__) ",true>", TF_FP16X2 | TF_PLANES | TF_GATHERED | TF_GROUPED, launch_conv3g<__VA_ARGS__, true>)
#define SAGEN_TILE_FAM_P3GH_MM(USE, id, ...) USE(id, "conv3g_kernel<" SAGEN_TILE_STR(__VA_ARGS__) ",true,1>", TF_FP16X2 | TF_PLANES | TF_GATHERED | TF_GROUPED | TF_FUSED_TAIL, launch_conv3g<__VA_ARGS__, true, 1>)
#define SAGEN_TILE_FAM_P3H(USE, id, ...)     USE(id, "conv3h_kernel<" SAGEN_TILE_STR(__VA_ARGS__) ">", TF_FP16X2 | TF_PLANES | TF_SHARED_TAPS | TF_GROUPED | TF_DH_SPLIT, launch_conv3h<__VA_ARGS__>)
#define SAGEN_TILE_FAM_P3HR(USE, id, ...)    USE(id, "conv3hr_kernel<" SAGEN_TILE_STR(__VA_ARGS__) ">", TF_FP16X2 | TF_PLANES | TF_SHARED_TAPS | TF_GROUPED | TF_RING3, launch_conv3h<__VA_ARGS__, 3>)
#define SAGEN_TILE_FAM_P3S(USE, id, ...)     USE(id, "conv3h_kernel<" SAGEN_TILE_STR(__VA_ARGS__) ",true>", TF_FP16X2 | TF_PLANES | TF_S2D | TF_GROUPED, launch_conv3s<__VA_ARGS__>)
#define SAGEN_TILE_UNWRAP(...) __VA_ARGS__

// The `case` lines of a dispatcher: a *_dispatch marks the families it launches (#define SAGEN_TILE_HAS_P3HR ,) and expands
// SAGEN_TILES(SAGEN_TILE_CASE) inside its switch - `case TILE_<id>: return <launch>(d, s);` for every row of a marked family, nothing
// for the rows of the others (the marker's comma moves the family's line into SAGEN_TILE_SECOND's place, else SAGEN_TILE_SKIP is there)
#define SAGEN_TILE_SKIP(...)
#define SAGEN_TILE_SECOND(a, b, ...) b
#define SAGEN_TILE_PICK(...) SAGEN_TILE_SECOND(__VA_ARGS__)
#define SAGEN_TILE_CASE_USE(id, name, traits, ...) case TILE_##id: return __VA_ARGS__(d, s);
#define SAGEN_TILE_CASE(id, fam, args, ...) SAGEN_TILE_PICK(SAGEN_TILE_HAS_##fam SAGEN_TILE_FAM_##fam, SAGEN_TILE_SKIP, )(SAGEN_TILE_CASE_USE, id, SAGEN_TILE_UNWRAP args)
