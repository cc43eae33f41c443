// A Python-free caller of the WHOLE inference chain through the C ABI (include/polyhead.h): from the image tensor to the panoptic id
// map and the depth maps -- fpn_c's program with the backbone in front.  It folds and packs the backbone's parameters on the device
// (ph_resnet_pack), creates the native backbone plan and runs it (ph_resnet_plan_run: one call, 57 launches at depth 50) into the
// stages ph_fpn_io.stages takes; the rest is fpn_c's: FPN plan -> neck plan's level inputs -> ph_neck_plan_run_outputs ->
// ph_khead_plan_run -> ph_decode_run -> ph_upsample2x -> ph_panoptic_merge, once, on one stream.  Links libpolyhead.so and the HIP
// runtime only.
//
//   image_main IN_DIR OUT_DIR
//
// IN_DIR/cfg.txt      fpn_c's 39 values (examples/fpn_c/fpn_main.cpp; k_l and h_l w_l must be the backbone's stage widths and sizes,
//                     x_dtype is the stages' element type), then 4 integers and a real:
//                       H W depth image_dtype bn_eps
//                     (the image size, the backbone's depth, PH_OUT_* of the image, the BatchNorm eps of the fold)
// IN_DIR/resnet.bin   the backbone's parameters, fp32, concatenated in the order of ph_resnet_param_name
// IN_DIR/image.bin    the image, image_dtype [B][3][H][W]
// IN_DIR/fpn.bin, neck.bin, khead.bin, stage<s>.bin   as fpn_c
// OUT_DIR/            s0 s1 s2 s3: the stages [B][k_l][h_l][w_l] of x_dtype; then fpn_c's files; geometry.txt with the backbone's lines
//                     in front
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/polyhead.h"

#define HIP_OK(x)                                                                          \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) {                                                            \
            std::fprintf(stderr, "%s:%d: %s: %s\n", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
            std::exit(2);                                                                  \
        }                                                                                  \
    } while (0)
#define PH_OK_(x)                                                                          \
    do {                                                                                   \
        int r_ = (x);                                                                      \
        if (r_ != PH_OK) {                                                                 \
            std::fprintf(stderr, "%s failed (%d): %s\n", #x, r_, ph_last_error_string());  \
            std::exit(3);                                                                  \
        }                                                                                  \
    } while (0)

static std::vector<char> read_file(const std::string& path, size_t expect) {
    FILE* f = std::fopen(path.c_str(), "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path.c_str()); std::exit(1); }
    std::vector<char> buf(expect);
    const size_t got = std::fread(buf.data(), 1, expect, f);
    const bool extra = std::fgetc(f) != EOF;
    std::fclose(f);
    if (got != expect || extra) { std::fprintf(stderr, "%s: expected %zu bytes\n", path.c_str(), expect); std::exit(1); }
    return buf;
}

static std::vector<void*> g_allocs;

static void* dev_alloc(size_t bytes, bool zero = false) {
    void* d = nullptr;
    HIP_OK(hipMalloc(&d, bytes ? bytes : 1));
    if (zero) HIP_OK(hipMemset(d, 0, bytes));
    g_allocs.push_back(d);
    return d;
}

static void* to_device(const std::vector<char>& h) {
    void* d = dev_alloc(h.size());
    HIP_OK(hipMemcpy(d, h.data(), h.size(), hipMemcpyHostToDevice));
    return d;
}

struct Out { std::string name; void* ptr; size_t bytes; };
static std::vector<Out> g_outs;

static void* out_alloc(const char* name, size_t bytes) {
    void* d = dev_alloc(bytes);
    g_outs.push_back({name, d, bytes});
    return d;
}

static void write_output(const std::string& path, const void* dev, size_t bytes) {
    std::vector<char> h(bytes);
    HIP_OK(hipMemcpy(h.data(), dev, bytes, hipMemcpyDeviceToHost));
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(h.data(), 1, bytes, f) != bytes) { std::fprintf(stderr, "cannot write %s\n", path.c_str()); std::exit(1); }
    std::fclose(f);
}

int main(int argc, char** argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s IN_DIR OUT_DIR\n", argv[0]); return 1; }
    const std::string in = argv[1], out = argv[2];
    ph_neck_cfg nc = {};             // every knob on auto: the module API's geometry
    ph_fpn_cfg fc = {};
    ph_resnet_cfg rc = {};
    ph_khead_cfg kc = {};
    ph_decode_cfg dc = {};
    int num_feats = 0, max_per_img = 0, depth_mode = 0, geom[8] = {};
    double score_thr = 0, overlap_thr = 0;
    {
        FILE* f = std::fopen((in + "/cfg.txt").c_str(), "r");
        if (!f || std::fscanf(f, "%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %lf %lf %d %d %d %d %d %d %d %d %d %d %lf",
                              &nc.B, &nc.h[0], &nc.w[0], &nc.h[1], &nc.w[1], &nc.h[2], &nc.w[2], &nc.h[3], &nc.w[3], &nc.groups, &nc.mode,
                              &nc.pos_level, &num_feats, &kc.num_proposals, &kc.num_classes, &kc.num_thing_classes, &dc.S, &dc.F, &dc.mode,
                              &dc.out_dtype, &dc.frame_invariant, &max_per_img, &depth_mode, &geom[0], &geom[1], &geom[2], &geom[3],
                              &geom[4], &geom[5], &geom[6], &geom[7], &score_thr, &overlap_thr, &fc.k[0], &fc.k[1], &fc.k[2], &fc.k[3], &fc.x_dtype,
                              &nc.tower_buffers, &rc.H, &rc.W, &rc.depth, &rc.x_dtype, &rc.eps) != 44) {
            std::fprintf(stderr, "cannot read %s/cfg.txt\n", in.c_str());
            return 1;
        }
        std::fclose(f);
    }
    nc.num_outs = 3;
    nc.emit_planes = 1;              // the KernelHead plan takes the planes: no fp32 map is written between the two
    fc.B = nc.B; fc.mode = nc.mode;
    for (int l = 0; l < 4; ++l) { fc.h[l] = nc.h[l]; fc.w[l] = nc.w[l]; }
    fc.emit_f32 = 1;                 // for p0 .. p3.bin; the neck reads the planes
    fc.emit_planes = 1;
    kc.B = nc.B; kc.H = nc.h[1]; kc.W = nc.w[1]; kc.groups = nc.groups; kc.mode = nc.mode;
    kc.cat_stuff = 1;
    kc.logit_dtype = PH_OUT_F32;
    kc.frame_invariant = dc.frame_invariant;
    if (nc.pos_level >= 0 && 2 * num_feats != 256) { std::fprintf(stderr, "num_feats must be 128 (256 channels)\n"); return 1; }
    hipStream_t stream;
    HIP_OK(hipStreamCreate(&stream));

    // 0b. the backbone: fold + pack (once per weight load), plan; its outputs are the FPN's stages
    rc.B = nc.B; rc.mode = nc.mode; rc.out_dtype = fc.x_dtype; rc.out_mask = 15;
    const size_t rpack_bytes = ph_resnet_pack_bytes(&rc), rws_bytes = ph_resnet_plan_workspace_bytes(&rc);
    if (!rpack_bytes || !rws_bytes) { std::fprintf(stderr, "bad backbone cfg: %s\n", ph_last_error_string()); return 3; }
    void* rpack = dev_alloc(rpack_bytes);
    {
        const int n = ph_resnet_nparams(&rc);
        size_t total = 0;
        for (int i = 0; i < n; ++i) total += (size_t)ph_resnet_param_numel(&rc, i) * 4;
        char* d = (char*)to_device(read_file(in + "/resnet.bin", total));
        std::vector<const float*> p(n);
        for (int i = 0; i < n; ++i) {
            p[i] = (const float*)d;
            d += (size_t)ph_resnet_param_numel(&rc, i) * 4;
        }
        PH_OK_(ph_resnet_pack(&rc, p.data(), rpack, stream));
    }
    void* rws = dev_alloc(rws_bytes);
    ph_resnet_plan* rplan = nullptr;
    PH_OK_(ph_resnet_plan_create(&rc, rpack, rws, rws_bytes, &rplan));
    ph_resnet_geometry rg;
    PH_OK_(ph_resnet_plan_info(rplan, &rg));
    for (int l = 0; l < 4; ++l)
        if (rg.c[l] != fc.k[l] || rg.h[l] != nc.h[l] || rg.w[l] != nc.w[l]) {
            std::fprintf(stderr, "stage %d is [%d][%d][%d], cfg.txt says [%d][%d][%d]\n", l, rg.c[l], rg.h[l], rg.w[l], fc.k[l], nc.h[l], nc.w[l]);
            return 3;
        }
    ph_resnet_io rio = {};
    rio.image = to_device(read_file(in + "/image.bin", (size_t)rc.B * 3 * rc.H * rc.W * (rc.x_dtype == PH_OUT_F32 ? 4 : 2)));

    // 0. the neck: positional encoding (once per map size), pack (once per weight load), plan; no zeroing contract
    const size_t npack_bytes = ph_neck_pack_bytes(&nc), nws_bytes = ph_neck_plan_workspace_bytes(&nc);
    if (!npack_bytes || !nws_bytes) { std::fprintf(stderr, "bad neck cfg: %s\n", ph_last_error_string()); return 3; }
    void* npack = dev_alloc(npack_bytes);
    {
        size_t total = 0;
        for (int i = 0; i < PH_NECK_NPARAMS; ++i) total += (size_t)ph_neck_param_numel(&nc, i) * 4;
        char* d = (char*)to_device(read_file(in + "/neck.bin", total));
        std::vector<const float*> p(PH_NECK_NPARAMS);
        for (int i = 0; i < PH_NECK_NPARAMS; ++i) {
            p[i] = (const float*)d;
            d += (size_t)ph_neck_param_numel(&nc, i) * 4;
        }
        PH_OK_(ph_neck_pack(&nc, p.data(), npack, stream));
    }
    void* nws = dev_alloc(nws_bytes);
    ph_neck_plan* nplan = nullptr;
    PH_OK_(ph_neck_plan_create(&nc, npack, nws, nws_bytes, &nplan));
    ph_neck_geometry ng;
    PH_OK_(ph_neck_plan_info(nplan, &ng));
    ph_neck_io nio = {};             // feats stay NULL: the towers start from the planes the FPN writes

    // 0a. the FPN: pack (once per weight load), plan; its outputs are the neck plan's level inputs and the fp32 levels
    const size_t fpack_bytes = ph_fpn_pack_bytes(&fc), fws_bytes = ph_fpn_plan_workspace_bytes(&fc);
    if (!fpack_bytes || !fws_bytes) { std::fprintf(stderr, "bad FPN cfg: %s\n", ph_last_error_string()); return 3; }
    void* fpack = dev_alloc(fpack_bytes);
    {
        size_t total = 0;
        for (int i = 0; i < PH_FPN_NPARAMS; ++i) total += (size_t)ph_fpn_param_numel(&fc, i) * 4;
        char* d = (char*)to_device(read_file(in + "/fpn.bin", total));
        std::vector<const float*> p(PH_FPN_NPARAMS);
        for (int i = 0; i < PH_FPN_NPARAMS; ++i) {
            p[i] = (const float*)d;
            d += (size_t)ph_fpn_param_numel(&fc, i) * 4;
        }
        PH_OK_(ph_fpn_pack(&fc, p.data(), fpack, stream));
    }
    void* fws = dev_alloc(fws_bytes);
    ph_fpn_plan* fplan = nullptr;
    PH_OK_(ph_fpn_plan_create(&fc, fpack, fws, fws_bytes, &fplan));
    ph_fpn_geometry fg;
    PH_OK_(ph_fpn_plan_info(fplan, &fg));
    if (fg.P != ng.P || fg.prec != ng.prec) { std::fprintf(stderr, "the neck does not read the FPN's planes\n"); return 3; }
    ph_fpn_io fio = {};
    const size_t xsz = fc.x_dtype == PH_OUT_F32 ? 4 : 2;
    for (int l = 0; l < 4; ++l) {
        fio.stages[l] = rio.stages[l] = out_alloc(("s" + std::to_string(l)).c_str(), (size_t)fc.B * fc.k[l] * fc.h[l] * fc.w[l] * xsz);
        fio.out_f32[l] = (float*)out_alloc(("p" + std::to_string(l)).c_str(), (size_t)fc.B * 256 * fc.h[l] * fc.w[l] * 4);
        int32_t prec_layout = 0;
        PH_OK_(ph_neck_plan_level_input(nplan, l, &fio.out_planes[l], &prec_layout));
        fio.planes_layout[l] = prec_layout & PH_PLANES_C16;
    }
    if (nc.pos_level >= 0) {
        float* pe = (float*)out_alloc("posenc", (size_t)256 * nc.h[nc.pos_level] * nc.w[nc.pos_level] * 4);
        PH_OK_(ph_neck_posenc(nc.h[nc.pos_level], nc.w[nc.pos_level], num_feats, 10000.0, 2 * 3.14159265358979323846, 1e-6, pe, stream));
        nio.posenc = pe;
        fio.add[nc.pos_level] = pe;  // the writer of a level's planes adds the positional encoding
    }
    for (int i = 0; i < 3; ++i)
        nio.out_planes[i] = (uint16_t*)out_alloc(("n" + std::to_string(i)).c_str(), (size_t)ng.P * nc.B * 256 * ng.HWp * 2);

    // 1. KernelHead: pack (once per weight load), workspace zeroed ONCE, plan
    const size_t kpack_bytes = ph_khead_pack_bytes(&kc);
    if (!kpack_bytes) { std::fprintf(stderr, "bad KernelHead cfg: %s\n", ph_last_error_string()); return 3; }
    void* kpack = dev_alloc(kpack_bytes);
    {
        size_t total = 0;
        for (int i = 0; i < PH_KHEAD_NPARAMS; ++i) total += (size_t)ph_khead_param_numel(&kc, i) * 4;
        char* d = (char*)to_device(read_file(in + "/khead.bin", total));
        std::vector<const float*> p(PH_KHEAD_NPARAMS);
        for (int i = 0; i < PH_KHEAD_NPARAMS; ++i) {
            p[i] = (const float*)d;
            d += (size_t)ph_khead_param_numel(&kc, i) * 4;
        }
        PH_OK_(ph_khead_pack(&kc, p.data(), kpack, stream));
    }
    const size_t kws_bytes = ph_khead_plan_workspace_bytes(&kc);
    if (!kws_bytes) { std::fprintf(stderr, "bad KernelHead cfg: %s\n", ph_last_error_string()); return 3; }
    void* kws = dev_alloc(kws_bytes, true);
    ph_khead_plan* kplan = nullptr;
    PH_OK_(ph_khead_plan_create(&kc, kpack, kws, kws_bytes, &kplan));
    ph_khead_geometry kg;
    PH_OK_(ph_khead_plan_info(kplan, &kg));
    if (kg.P != ng.P || kg.prec != ng.prec || kg.HWp != ng.HWp) { std::fprintf(stderr, "KernelHead does not read the neck's planes\n"); return 3; }

    // 2. the decode: N, L and the frame geometry follow from KernelHead's
    dc.B = kc.B; dc.N = kg.N; dc.H = kc.H; dc.W = kc.W; dc.L = kc.num_classes;
    const size_t dpack_bytes = ph_decode_pack_bytes(&dc);
    if (!dpack_bytes) { std::fprintf(stderr, "bad decode cfg: %s\n", ph_last_error_string()); return 3; }
    std::vector<void*> packs(dc.S);
    for (int s = 0; s < dc.S; ++s) {
        size_t total = 0;
        for (int i = 0; i < PH_DECODE_NPARAMS; ++i) total += (size_t)ph_decode_param_numel(&dc, i) * 4;
        char* d = (char*)to_device(read_file(in + "/stage" + std::to_string(s) + ".bin", total));
        std::vector<const float*> p(PH_DECODE_NPARAMS);
        for (int i = 0; i < PH_DECODE_NPARAMS; ++i) {
            p[i] = (const float*)d;
            d += (size_t)ph_decode_param_numel(&dc, i) * 4;
        }
        packs[s] = dev_alloc(dpack_bytes);
        PH_OK_(ph_decode_pack_stage(&dc, p.data(), packs[s], stream));
    }
    const size_t dws_bytes = ph_decode_workspace_bytes(&dc);
    void* dws = dev_alloc(dws_bytes);
    ph_decode* dplan = nullptr;
    PH_OK_(ph_decode_create(&dc, (const void* const*)packs.data(), dws, dws_bytes, &dplan));
    ph_decode_geometry dg;
    PH_OK_(ph_decode_info(dplan, &dg));
    if (dg.feat_planes != kg.P || dg.feat_prec != kg.prec) {
        std::fprintf(stderr, "the decode mode does not read KernelHead's planes (a1 grade %d x %d planes, decode %d x %d)\n", kg.prec, kg.P,
                     dg.feat_prec, dg.feat_planes);
        return 3;
    }

    // 3. caller-owned outputs
    const size_t B = kc.B, N = kg.N, HW = (size_t)kc.H * kc.W, HWp = kg.HWp, ob = dc.out_dtype == PH_OUT_F32 ? 4 : 2, L = kc.num_classes;
    ph_khead_io kio = {};
    kio.input_format = PH_IN_PLANES;
    kio.f0 = nio.out_planes[0];
    kio.f1 = nio.out_planes[1];
    kio.f2 = nio.out_planes[2];
    kio.xp = (uint16_t*)out_alloc("xp", (size_t)kg.P * B * 256 * HWp * 2);
    kio.dp = (uint16_t*)out_alloc("dp", (size_t)kg.P * B * 256 * HWp * 2);
    kio.bits = (uint32_t*)out_alloc("bits", B * kg.Npad * (HWp / 32) * 4);
    kio.mask_preds = out_alloc("mask_preds", B * N * HW * 4);
    kio.seg_preds = out_alloc("seg_preds", B * L * HW * 4);
    kio.depth_pred = out_alloc("depth_pred", B * HW * 4);
    kio.proposal = (float*)out_alloc("proposal", B * N * 256 * 4);
    kio.depth_proposal = (float*)out_alloc("depth_proposal", B * N * 256 * 4);

    ph_decode_io dio = {};
    dio.feat_format = PH_FEAT_PLANES;
    dio.x = kio.xp;
    dio.depth_feats = kio.dp;
    dio.bits = kio.bits;
    dio.k0 = kio.proposal;
    dio.q0 = kio.depth_proposal;
    dio.obj = (float*)out_alloc("obj", B * N * 256 * 4);
    dio.dobj = (float*)out_alloc("dobj", B * N * 256 * 4);
    dio.cls = (float*)out_alloc("cls", B * N * L * 4);
    dio.mask = out_alloc("mask", B * N * HW * ob);
    dio.mask_up = out_alloc("mask_up", B * N * HW * 4 * ob);
    dio.depth_up = out_alloc("depth_up", B * N * HW * 4 * ob);

    const int h2 = 2 * kc.H, w2 = 2 * kc.W;
    float* depth_init_up = (float*)out_alloc("depth_init_up", B * HW * 4 * 4);
    const int n_stuff_q = (int)N - kc.num_proposals, n_stuff_c = kc.num_classes - kc.num_thing_classes;
    const int K = max_per_img + (n_stuff_q < n_stuff_c ? n_stuff_q : n_stuff_c);
    const size_t mws_bytes = ph_panoptic_merge_workspace_bytes(kc.B, K, h2, w2, geom);
    if (!mws_bytes) { std::fprintf(stderr, "bad merge geometry: %s\n", ph_last_error_string()); return 3; }
    void* mws = dev_alloc(mws_bytes);
    const size_t opx = (size_t)geom[6] * geom[7];
    int32_t* pan = (int32_t*)out_alloc("pan", B * opx * 4);
    float* depth_basic = (float*)out_alloc("depth_basic", B * opx * 4);
    float* depth_final = (float*)out_alloc("depth_final", B * opx * 4);
    int32_t* seg_records = (int32_t*)out_alloc("seg_records", B * (1 + 5 * (size_t)K) * 4);

    // 4. one frame batch: native calls, launches only; the first failure ends the program
    PH_OK_(ph_resnet_plan_run(rplan, &rio, stream));
    if (ng.tower_buffers) {          // every level owns its input planes: the whole FPN, then the four towers
        PH_OK_(ph_fpn_plan_run(fplan, &fio, stream));
        for (int l = 0; l < 4; ++l) PH_OK_(ph_neck_plan_run_level_planes(nplan, l, stream));
    } else {                         // one shared input buffer: a level's tower runs before the next level is written
        PH_OK_(ph_fpn_plan_run_laterals(fplan, &fio, stream));
        for (int l = 0; l < 4; ++l) {
            PH_OK_(ph_fpn_plan_run_output(fplan, l, &fio, stream));
            PH_OK_(ph_neck_plan_run_level_planes(nplan, l, stream));
        }
    }
    PH_OK_(ph_neck_plan_run_outputs(nplan, &nio, stream));
    PH_OK_(ph_khead_plan_run(kplan, &kio, stream));
    PH_OK_(ph_decode_run(dplan, &dio, stream));
    PH_OK_(ph_upsample2x(kio.depth_pred, depth_init_up, PH_OUT_F32, (int64_t)B, kc.H, kc.W, stream));
    PH_OK_(ph_panoptic_merge(dio.cls, dio.mask_up, dio.depth_up, dc.out_dtype, depth_init_up, kc.B, (int)N, (int)L, kc.num_proposals,
                             kc.num_thing_classes, max_per_img, h2, w2, geom, depth_mode, score_thr, overlap_thr, mws, mws_bytes, pan,
                             depth_basic, depth_final, seg_records, stream));
    HIP_OK(hipStreamSynchronize(stream));
    const int fell_back = ph_khead_plan_status(kplan, stream), timeouts = ph_khead_plan_timeouts(kplan, stream);
    if (fell_back < 0 || timeouts < 0) { std::fprintf(stderr, "cannot read the KernelHead plan's status\n"); return 3; }
    for (const Out& o : g_outs) write_output(out + "/" + o.name + ".bin", o.ptr, o.bytes);
    FILE* g = std::fopen((out + "/geometry.txt").c_str(), "w");
    if (!g) { std::fprintf(stderr, "cannot write %s/geometry.txt\n", out.c_str()); return 1; }
    std::fprintf(g, "resnet_prec %d\nresnet_launches %d\nresnet_nconvs %d\nresnet_stem_workgroups %d\n", rg.prec, rg.launches, rg.nconvs,
                 rg.stem_workgroups);
    std::fprintf(g, "fpn_P %d\nfpn_prec %d\nfpn_tile_rows_0 %d\nfpn_tile_rows_1 %d\nfpn_tile_rows_2 %d\nfpn_tile_rows_3 %d\nneck_tower_buffers %d\n", fg.P, fg.prec, fg.tile_rows[0], fg.tile_rows[1],
                 fg.tile_rows[2], fg.tile_rows[3], ng.tower_buffers);
    std::fprintf(g, "neck_fused_out %d\nneck_c16 %d\nneck_P %d\nneck_HWp %d\n", ng.fused_out, ng.c16, ng.P, ng.HWp);
    std::fprintf(g, "khead_onepass %d\nkhead_nsplit %d\nN %d\nNpad %d\nHWp %d\nP %d\nkhead_prec %d\nfell_back %d\ntimeouts %d\n", kg.onepass,
                 kg.nsplit, kg.N, kg.Npad, kg.HWp, kg.P, kg.prec, fell_back, timeouts);
    std::fprintf(g, "nsplit %d\nnsplit_px %d\npoolx %d\nfused_up %d\nup2_workgroups %d\nK %d\n", dg.nsplit, dg.nsplit_px, dg.poolx,
                 dg.fused_up, dg.up2_workgroups, K);
    std::fclose(g);

    ph_decode_destroy(dplan);
    ph_khead_plan_destroy(kplan);
    ph_neck_plan_destroy(nplan);
    ph_fpn_plan_destroy(fplan);
    ph_resnet_plan_destroy(rplan);
    for (void* p : g_allocs) HIP_OK(hipFree(p));
    HIP_OK(hipStreamDestroy(stream));
    std::printf("backbone + fpn + neck + head: %d frame(s), neck fused_out %d c16 %d, N %d, one-pass %d (fell back %d), decode nsplit %d poolx %d "
                "fused_up %d, K %d\n", kc.B, ng.fused_out, ng.c16, kg.N, kg.onepass, fell_back, dg.nsplit, dg.poolx, dg.fused_up, K);
    return 0;
}
