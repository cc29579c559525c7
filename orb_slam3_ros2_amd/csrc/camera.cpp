// Distorted pinhole camera, host side (beside camera_kernels.hip): the host calls of
// Frame::UndistortKeyPoints and ComputeImageBounds with their scratch.
#include "devbuf.h"
#include "orbhip_kernels.h"
#include "stage.h"

#define HIPOK(x) ORBHIP_HIPOK(" camera", x)

namespace orbhip {

struct CameraWorkspace {
    DevBuf<orbhip_kp> d_kps;   // undistorted in place
    DevBuf<float> d_bounds;
};
CameraWorkspace* camera_ws_create() { return new CameraWorkspace(); }
void camera_ws_destroy(CameraWorkspace* ws) { delete ws; }

int undistort_kps_host(CameraWorkspace* ws, const orbhip_pinhole& cam, const orbhip_kp* kps, int n, orbhip_kp* out,
                       hipStream_t st) {
    HIPOK(ws->d_kps.ensure((size_t)n));
    HIPOK(hipMemcpyAsync(ws->d_kps.p, kps, sizeof(orbhip_kp) * (size_t)n, hipMemcpyHostToDevice, st));
    (void)hipGetLastError();
    launch_undistort_kps(ws->d_kps.p, nullptr, n, 1, n, cam, ws->d_kps.p, st);
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpyAsync(out, ws->d_kps.p, sizeof(orbhip_kp) * (size_t)n, hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    return ORBHIP_OK;
}

int image_bounds_host(CameraWorkspace* ws, const orbhip_pinhole& cam, int cols, int rows, float bounds[4],
                      hipStream_t st) {
    HIPOK(ws->d_bounds.ensure(4));
    (void)hipGetLastError();
    launch_image_bounds(cols, rows, cam, ws->d_bounds.p, st);
    HIPOK(hipGetLastError());
    HIPOK(hipMemcpyAsync(bounds, ws->d_bounds.p, 4 * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPOK(hipStreamSynchronize(st));
    return ORBHIP_OK;
}

}  // namespace orbhip
