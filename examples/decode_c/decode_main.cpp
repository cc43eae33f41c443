// A Python-free caller of the native decode plan (include/polyhead.h ph_decode_*): reads raw fp32 weights and inputs, packs
// every stage on the device, creates a plan, runs it once on a stream and writes the outputs.  Links libpolyhead.so and the
// HIP runtime only.
//
//   decode_main IN_DIR OUT_DIR
//
// IN_DIR/cfg.txt         "B N H W S L F mode out_dtype frame_invariant" (integers; mode = PH_MODE_*, out_dtype = PH_OUT_*)
// IN_DIR/stage<s>.bin    stage s's parameters, fp32, concatenated in the order of polyhead.h's table (ph_decode_param_numel)
// IN_DIR/x.bin, depth_feats.bin   fp32 [B][256][H][W];   k0.bin, q0.bin   fp32 [B][N][256];   m0.bin   fp32 [B][N][H][W]
// OUT_DIR/{obj,dobj,cls,mask,mask_up,depth_up}.bin   raw outputs (fp32 / out_dtype), and geometry.txt
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

static void* to_device(const std::vector<char>& h) {
    void* d = nullptr;
    HIP_OK(hipMalloc(&d, h.size()));
    HIP_OK(hipMemcpy(d, h.data(), h.size(), hipMemcpyHostToDevice));
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
    ph_decode_cfg cfg = {};          // every knob on auto: the module API's geometry
    {
        FILE* f = std::fopen((in + "/cfg.txt").c_str(), "r");
        if (!f || std::fscanf(f, "%d %d %d %d %d %d %d %d %d %d", &cfg.B, &cfg.N, &cfg.H, &cfg.W, &cfg.S, &cfg.L, &cfg.F, &cfg.mode,
                              &cfg.out_dtype, &cfg.frame_invariant) != 10) {
            std::fprintf(stderr, "cannot read %s/cfg.txt\n", in.c_str());
            return 1;
        }
        std::fclose(f);
    }
    const size_t B = cfg.B, N = cfg.N, HW = (size_t)cfg.H * cfg.W, ob = cfg.out_dtype == PH_OUT_F32 ? 4 : 2;
    hipStream_t stream;
    HIP_OK(hipStreamCreate(&stream));

    // 1. pack every stage (once per weight load)
    const size_t pack_bytes = ph_decode_pack_bytes(&cfg);
    if (!pack_bytes) { std::fprintf(stderr, "bad cfg: %s\n", ph_last_error_string()); return 3; }
    std::vector<void*> packs(cfg.S), params_dev;
    for (int s = 0; s < cfg.S; ++s) {
        size_t total = 0;
        for (int i = 0; i < PH_DECODE_NPARAMS; ++i) total += (size_t)ph_decode_param_numel(&cfg, i) * 4;
        const std::vector<char> h = read_file(in + "/stage" + std::to_string(s) + ".bin", total);
        char* d = (char*)to_device(h);
        params_dev.push_back(d);
        std::vector<const float*> p(PH_DECODE_NPARAMS);
        for (int i = 0; i < PH_DECODE_NPARAMS; ++i) {
            p[i] = (const float*)d;
            d += (size_t)ph_decode_param_numel(&cfg, i) * 4;
        }
        HIP_OK(hipMalloc(&packs[s], pack_bytes));
        PH_OK_(ph_decode_pack_stage(&cfg, p.data(), packs[s], stream));
    }

    // 2. the plan: caller-owned workspace
    const size_t ws_bytes = ph_decode_workspace_bytes(&cfg);
    void* ws = nullptr;
    HIP_OK(hipMalloc(&ws, ws_bytes));
    ph_decode* plan = nullptr;
    PH_OK_(ph_decode_create(&cfg, (const void* const*)packs.data(), ws, ws_bytes, &plan));
    ph_decode_geometry geo;
    PH_OK_(ph_decode_info(plan, &geo));

    // 3. inputs and caller-owned outputs
    ph_decode_io io = {};
    io.feat_format = PH_FEAT_F32;
    io.m0_dtype = PH_OUT_F32;
    io.x = to_device(read_file(in + "/x.bin", B * 256 * HW * 4));
    io.depth_feats = to_device(read_file(in + "/depth_feats.bin", B * 256 * HW * 4));
    io.k0 = (const float*)to_device(read_file(in + "/k0.bin", B * N * 256 * 4));
    io.q0 = (const float*)to_device(read_file(in + "/q0.bin", B * N * 256 * 4));
    io.m0 = to_device(read_file(in + "/m0.bin", B * N * HW * 4));
    struct Out { const char* name; void** ptr; size_t bytes; };
    const Out outs[] = {{"obj", (void**)&io.obj, B * N * 256 * 4}, {"dobj", (void**)&io.dobj, B * N * 256 * 4},
                        {"cls", (void**)&io.cls, B * N * cfg.L * 4}, {"mask", &io.mask, B * N * HW * ob},
                        {"mask_up", &io.mask_up, B * N * HW * 4 * ob}, {"depth_up", &io.depth_up, B * N * HW * 4 * ob}};
    for (const Out& o : outs) HIP_OK(hipMalloc(o.ptr, o.bytes));

    // 4. one decode
    PH_OK_(ph_decode_run(plan, &io, stream));
    HIP_OK(hipStreamSynchronize(stream));
    for (const Out& o : outs) write_output(out + "/" + o.name + ".bin", *o.ptr, o.bytes);
    FILE* g = std::fopen((out + "/geometry.txt").c_str(), "w");
    if (g) {
        std::fprintf(g, "nsplit %d\nnsplit_px %d\npoolx %d\nfused_up %d\nup2_workgroups %d\n", geo.nsplit, geo.nsplit_px, geo.poolx,
                     geo.fused_up, geo.up2_workgroups);
        std::fclose(g);
    }

    ph_decode_destroy(plan);
    for (const Out& o : outs) HIP_OK(hipFree(*o.ptr));
    for (const void* p : {io.x, io.depth_feats, (const void*)io.k0, (const void*)io.q0, io.m0}) HIP_OK(hipFree((void*)p));
    for (void* p : packs) HIP_OK(hipFree(p));
    for (void* p : params_dev) HIP_OK(hipFree(p));
    HIP_OK(hipFree(ws));
    HIP_OK(hipStreamDestroy(stream));
    std::printf("decoded %d frame(s): nsplit %d, poolx %d, fused_up %d\n", cfg.B, geo.nsplit, geo.poolx, geo.fused_up);
    return 0;
}
