// The stereo stage, host side (stereo.h): the device form, the host-image form and the test hooks.
// Each runs behind an extraction (or a pyramid stage) of the same call and on the same stream, and
// reads the pyramids where that left them.
#include "stereo.h"

#include <algorithm>

#include "extract.h"
#include "stage.h"

#define HIPOK(x) ORBHIP_HIPOK(" stereo", x)

namespace orbhip {

static bool valid_params(const orbhip_stereo_params& p) { return p.bf > 0.0f && p.b > 0.0f; }

static StereoArgs stereo_args(const ExtractView& v, const orbhip_stereo_params& prm, int P, int cap) {
    StereoArgs a{};
    a.d_plan = v.d_plan;
    a.pyr = v.d_pyr;
    a.cap = cap;
    a.P = P;
    a.bf = prm.bf;
    a.b = prm.b;
    a.center_patch = prm.center_patch != 0;
    return a;
}

int stereo_device(ExtractWorkspace* ws, const uint8_t* d_imgs, int P, int w, int h, int stride, int64_t fstride,
                  const orbhip_stereo_params& prm, orbhip_kp* d_kps, uint8_t* d_desc, int cap, int32_t* d_n,
                  int32_t* d_mono, float* d_u_right, float* d_depth, int32_t* d_status, int32_t* d_n_stereo,
                  hipStream_t st) {
    if (!valid_params(prm)) return ORBHIP_ERR_ARG;
    ExtractView v;
    if (int rc = extract_view(ws, w, h, &v)) return rc;
    if (cap < v.kp_cap) return ORBHIP_ERR_CAPACITY;
    if (v.kp_cap > kStereoMaxKp) return ORBHIP_ERR_UNSUPPORTED;
    if (int rc = extract_batch(ws, d_imgs, 2 * P, w, h, stride, fstride, 0, 0, d_kps, d_desc, cap, d_n, d_mono, st))
        return rc;
    StereoScratch s;
    if (int rc = extract_stereo_scratch(ws, (size_t)P * cap, P, false, &s)) return rc;
    if (int rc = extract_view(ws, w, h, &v)) return rc;   // the pyramid block as the extraction left it
    StereoArgs a = stereo_args(v, prm, P, cap);
    a.img = d_imgs; a.stride = stride; a.fstride = fstride;
    a.kps = d_kps; a.desc = d_desc; a.n = d_n;
    a.u_right = d_u_right; a.depth = d_depth; a.status_out = d_status; a.n_stereo = d_n_stereo;
    a.status = s.status; a.sad = s.sad;
    (void)hipGetLastError();
    launch_stereo(a, st);
    HIPOK(hipGetLastError());
    return ORBHIP_OK;
}

int stereo_host(ExtractWorkspace* ws, const uint8_t* left, const uint8_t* right, int w, int h, int stride,
                const orbhip_stereo_params& prm, orbhip_kp* kps_l, uint8_t* desc_l, int* n_l, orbhip_kp* kps_r,
                uint8_t* desc_r, int* n_r, int cap, float* u_right, float* depth, int32_t* status, int* n_stereo) {
    if (!valid_params(prm)) return ORBHIP_ERR_ARG;
    ExtractView v;
    if (int rc = extract_view(ws, w, h, &v)) return rc;
    if (cap < v.kp_cap) return ORBHIP_ERR_CAPACITY;
    if (v.kp_cap > kStereoMaxKp) return ORBHIP_ERR_UNSUPPORTED;
    const int kcap = v.kp_cap;
    if (int rc = extract_host_pair(ws, left, right, w, h, stride, false)) return rc;
    StereoScratch s;
    if (int rc = extract_stereo_scratch(ws, (size_t)kcap, 1, true, &s)) return rc;
    if (int rc = extract_view(ws, w, h, &v)) return rc;
    hipStream_t st = v.stream;
    StereoArgs a = stereo_args(v, prm, 1, kcap);
    a.img = v.d_in; a.stride = w; a.fstride = (int64_t)w * h;
    a.kps = v.d_kps; a.desc = v.d_desc; a.n = v.d_n;
    a.u_right = s.u_right; a.depth = s.depth; a.status_out = nullptr; a.n_stereo = s.n_stereo;
    a.status = s.status; a.sad = s.sad;
    (void)hipGetLastError();
    launch_stereo(a, st);
    HIPOK(hipGetLastError());
    int n[2] = {0, 0}, err[4] = {0, 0, 0, 0}, nst = 0;
    HIPOK(hipMemcpyAsync(n, v.d_n, sizeof(n), hipMemcpyDeviceToHost, st));
    HIPOK(hipMemcpyAsync(err, v.d_err, sizeof(err), hipMemcpyDeviceToHost, st));
    HIPOK(hipMemcpyAsync(&nst, s.n_stereo, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    if (err[0]) return ORBHIP_ERR_DEVICE;
    *n_l = n[0];
    *n_r = n[1];
    if (n[0] > cap || n[1] > cap) return ORBHIP_ERR_CAPACITY;
    *n_stereo = nst;
    const size_t nl = (size_t)n[0], nr = (size_t)n[1];
    if (nl) {
        HIPOK(hipMemcpyAsync(kps_l, v.d_kps, nl * sizeof(orbhip_kp), hipMemcpyDeviceToHost, st));
        HIPOK(hipMemcpyAsync(desc_l, v.d_desc, nl * 32, hipMemcpyDeviceToHost, st));
        HIPOK(hipMemcpyAsync(u_right, s.u_right, nl * sizeof(float), hipMemcpyDeviceToHost, st));
        HIPOK(hipMemcpyAsync(depth, s.depth, nl * sizeof(float), hipMemcpyDeviceToHost, st));
        if (status) HIPOK(hipMemcpyAsync(status, s.status, nl * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    }
    if (nr) {
        HIPOK(hipMemcpyAsync(kps_r, v.d_kps + kcap, nr * sizeof(orbhip_kp), hipMemcpyDeviceToHost, st));
        HIPOK(hipMemcpyAsync(desc_r, v.d_desc + (size_t)kcap * 32, nr * 32, hipMemcpyDeviceToHost, st));
    }
    HIPOK(hipStreamSynchronize(st));
    return ORBHIP_OK;
}

namespace {
// the hook's own device arrays (freed when it returns)
struct Tmp {
    void* p = nullptr;
    ~Tmp() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, std::max<size_t>(bytes, 1)); }
};
}  // namespace

int stereo_test_match(ExtractWorkspace* ws, const uint8_t* left, const uint8_t* right, int w, int h,
                      const orbhip_stereo_params& prm, const orbhip_kp* kps_l, const uint8_t* desc_l, int n_l,
                      const orbhip_kp* kps_r, const uint8_t* desc_r, int n_r, float* u_right, float* depth,
                      int32_t* status, int32_t* best_r, int32_t* sad, int* n_stereo) {
    if (!valid_params(prm) || n_l < 0 || n_r < 0 || n_l > kStereoMaxKp || n_r > kStereoMaxKp) return ORBHIP_ERR_ARG;
    if (int rc = extract_host_pair(ws, left, right, w, h, w, true)) return rc;
    ExtractView v;
    if (int rc = extract_view(ws, w, h, &v)) return rc;
    hipStream_t st = v.stream;
    const int cap = std::max(std::max(n_l, n_r), 1);
    StereoScratch s;
    if (int rc = extract_stereo_scratch(ws, (size_t)cap, 1, true, &s)) return rc;
    Tmp d_kps, d_desc, d_n;
    HIPOK(d_kps.alloc((size_t)2 * cap * sizeof(orbhip_kp)));
    HIPOK(d_desc.alloc((size_t)2 * cap * 32));
    HIPOK(d_n.alloc(2 * sizeof(int32_t)));
    const int32_t n[2] = {n_l, n_r};
    HIPOK(hipMemcpyAsync(d_n.p, n, sizeof(n), hipMemcpyHostToDevice, st));
    if (n_l) {
        HIPOK(hipMemcpyAsync(d_kps.p, kps_l, (size_t)n_l * sizeof(orbhip_kp), hipMemcpyHostToDevice, st));
        HIPOK(hipMemcpyAsync(d_desc.p, desc_l, (size_t)n_l * 32, hipMemcpyHostToDevice, st));
    }
    if (n_r) {
        HIPOK(hipMemcpyAsync((orbhip_kp*)d_kps.p + cap, kps_r, (size_t)n_r * sizeof(orbhip_kp), hipMemcpyHostToDevice,
                             st));
        HIPOK(hipMemcpyAsync((uint8_t*)d_desc.p + (size_t)cap * 32, desc_r, (size_t)n_r * 32, hipMemcpyHostToDevice,
                             st));
    }
    StereoArgs a = stereo_args(v, prm, 1, cap);
    a.img = v.d_in; a.stride = w; a.fstride = (int64_t)w * h;
    a.kps = (const orbhip_kp*)d_kps.p; a.desc = (const uint8_t*)d_desc.p; a.n = (const int32_t*)d_n.p;
    a.u_right = s.u_right; a.depth = s.depth; a.status_out = nullptr; a.n_stereo = s.n_stereo;
    a.status = s.status; a.sad = s.sad; a.best_r = s.best;
    (void)hipGetLastError();
    launch_stereo(a, st);
    HIPOK(hipGetLastError());
    const size_t nl = (size_t)n_l;
    if (nl) {
        HIPOK(hipMemcpyAsync(u_right, s.u_right, nl * 4, hipMemcpyDeviceToHost, st));
        HIPOK(hipMemcpyAsync(depth, s.depth, nl * 4, hipMemcpyDeviceToHost, st));
        HIPOK(hipMemcpyAsync(status, s.status, nl * 4, hipMemcpyDeviceToHost, st));
        HIPOK(hipMemcpyAsync(best_r, s.best, nl * 4, hipMemcpyDeviceToHost, st));
        HIPOK(hipMemcpyAsync(sad, s.sad, nl * 4, hipMemcpyDeviceToHost, st));
    }
    HIPOK(hipMemcpyAsync(n_stereo, s.n_stereo, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    return ORBHIP_OK;
}

int stereo_test_median(int32_t* status, const int32_t* sad, float* u_right, float* depth, int n, int* n_stereo) {
    if (n < 0 || n > kStereoMaxKp) return ORBHIP_ERR_ARG;
    const int cap = std::max(n, 1);
    const size_t bytes = (size_t)n * 4;
    Tmp d_status, d_sad, d_u, d_depth, d_n, d_nst;
    HIPOK(d_status.alloc((size_t)cap * 4));
    HIPOK(d_sad.alloc((size_t)cap * 4));
    HIPOK(d_u.alloc((size_t)cap * 4));
    HIPOK(d_depth.alloc((size_t)cap * 4));
    HIPOK(d_n.alloc(2 * sizeof(int32_t)));
    HIPOK(d_nst.alloc(sizeof(int32_t)));
    const int32_t nn[2] = {n, 0};
    HIPOK(hipMemcpy(d_n.p, nn, sizeof(nn), hipMemcpyHostToDevice));
    HIPOK(hipMemset(d_nst.p, 0xFF, sizeof(int32_t)));   // the kernel must write it, also with n == 0
    if (n) {
        HIPOK(hipMemcpy(d_status.p, status, bytes, hipMemcpyHostToDevice));
        HIPOK(hipMemcpy(d_sad.p, sad, bytes, hipMemcpyHostToDevice));
        HIPOK(hipMemcpy(d_u.p, u_right, bytes, hipMemcpyHostToDevice));
        HIPOK(hipMemcpy(d_depth.p, depth, bytes, hipMemcpyHostToDevice));
    }
    StereoArgs a{};
    a.cap = cap;
    a.P = 1;
    a.n = (const int32_t*)d_n.p;
    a.status = (int32_t*)d_status.p; a.sad = (int32_t*)d_sad.p;
    a.u_right = (float*)d_u.p; a.depth = (float*)d_depth.p; a.n_stereo = (int32_t*)d_nst.p;
    (void)hipGetLastError();
    launch_stereo_median(a, nullptr);
    HIPOK(hipGetLastError());
    HIPOK(hipDeviceSynchronize());
    if (n) {
        HIPOK(hipMemcpy(status, d_status.p, bytes, hipMemcpyDeviceToHost));
        HIPOK(hipMemcpy(u_right, d_u.p, bytes, hipMemcpyDeviceToHost));
        HIPOK(hipMemcpy(depth, d_depth.p, bytes, hipMemcpyDeviceToHost));
    }
    HIPOK(hipMemcpy(n_stereo, d_nst.p, sizeof(int), hipMemcpyDeviceToHost));
    return ORBHIP_OK;
}

}  // namespace orbhip
