// TEST INFRASTRUCTURE: host build of the two ray codes side by side -- the rangefinder rays of the step kernel
// (dm_control_amd/csrc/step_geom.h: ray_geom_any, on a world-frame pose) and the camera's (camera_core.h: cam_ray_local
// behind the camera's own pre-transform, cam_stage_geom + cam_pixel_geom).  Nothing else of the step core is included.
#define DMC_HOST_EMU 1
#include "../../dm_control_amd/csrc/step_geom.h"
#include "../../dm_control_amd/csrc/camera_core.h"

using namespace dmc;

// n rays (pnt, unit vec) against one geom each; distance or -1 from either code
extern "C" void geom_emu_rays(int n, const int* type, const double* size, const double* gpos, const double* gmat,
                              const double* pnt, const double* vec, double* t_step, double* t_cam) {
  for (int i = 0; i < n; i++) {
    const double *s = size + 3*i, *p = gpos + 3*i, *m = gmat + 9*i, *o = pnt + 3*i, *v = vec + 3*i;
    t_step[i] = ray_geom_any(p, m, s, o, v, type[i]);
    // the camera: origin at the ray's, looking along it -- the pixel on the axis (dx = dy = 0) sees R (0, 0, -1) = vec
    const double R[9] = {0, 0, -v[0], 0, 0, -v[1], 0, 0, -v[2]};
    CamGeom<double> e;
    cam_stage_geom(&e, p, m, s, type[i], i, o, R);
    CamHit<double> h;
    h.id = -1; h.t = 0; h.type = 0; h.part = 0;
    cam_pixel_geom(e, 0.0, 0.0, 0.0, (double)INFINITY, &h);
    t_cam[i] = h.id >= 0 ? h.t : -1;
  }
}
