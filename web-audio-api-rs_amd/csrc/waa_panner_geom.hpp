// waa_panner_geom.hpp — the geometry of one frame of the equal-power PannerNode under an audio-rate AudioListener
// (panner.rs:720-779 a_rate_params, :830-897; spatial.rs:205-299): what panner_geom_kernel (one option set per node, passed in the
// kernel's arguments) and panner_geom_inst_kernel (one set per instance, read from a table), both in waa_panner.hip, compute from
// a frame's fifteen param values.  Both evaluate this one function, so a context's gains do not depend on how its options reached
// the kernel.  Device code only; built like the rest of the library with -ffp-contract=off.
#ifndef WAA_PANNER_GEOM_HPP
#define WAA_PANNER_GEOM_HPP

#include <hip/hip_runtime.h>

#include <cfloat>

#include "waa_internal.hpp"

namespace waa {

namespace panner_geom {
struct V3 {
  float x, y, z;
};
__device__ __forceinline__ V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dot(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ float sqlen(V3 a) { return a.x * a.x + a.y * a.y + a.z * a.z; }
__device__ __forceinline__ V3 scale(V3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ V3 normalized(V3 a) { return scale(a, 1.f / sqrtf(sqlen(a))); }
__device__ __forceinline__ V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
constexpr float PI_F = 3.14159265358979323846f;

// spatial.rs:205-270
__device__ __forceinline__ void azimuth_elevation(V3 sp, V3 lp, V3 lf, V3 lu, float* az) {
  *az = 0.f;
  const V3 rel = sub(sp, lp);
  if (sqlen(rel) <= FLT_MIN) return;
  const V3 sl = normalized(rel);
  const V3 right = cross(lf, lu);
  if (sqlen(right) == 0.f) return;
  const V3 rn = normalized(right), fn = normalized(lf), up = cross(rn, fn);
  const float up_proj = dot(sl, up);
  const V3 ps = sub(sl, scale(up, up_proj));
  if (sqlen(ps) == 0.f) return;
  const V3 psn = normalized(ps);
  float azimuth = 180.f * acosf(dot(psn, rn)) / PI_F;
  if (dot(psn, fn) < 0.f) azimuth = 360.f - azimuth;
  if (azimuth >= 0.f && azimuth <= 270.f)
    azimuth = 90.f - azimuth;
  else
    azimuth = 450.f - azimuth;
  *az = azimuth;
}
// spatial.rs:278-299
__device__ __forceinline__ float spatial_angle(V3 sp, V3 so, V3 lp) {
  if (sqlen(so) == 0.f) return 0.f;
  const V3 son = normalized(so), rel = sub(sp, lp);
  if (sqlen(rel) <= FLT_MIN) return 0.f;
  const V3 sl = normalized(rel);
  return fabsf(180.f * acosf(dot(sl, son)) / PI_F);
}
}  // namespace panner_geom

// The geometry of one frame: the azimuth wrapped to [-90, 90], the equal-power gains of the mono and the stereo law, the distance
// gain and the cone gain.
struct PannerGeomOut {
  float az, gl_mono, gr_mono, gl_stereo, gr_stereo, dg, cg;
};

// One frame's geometry from the fifteen param values v (WAA_PARAM_PANNER_* / WAA_PARAM_LISTENER_* in id order) and the option set
// `o`.  Nothing here assumes that the threads of a block share `o`: a block may straddle two table rows.
__device__ __forceinline__ PannerGeomOut panner_geom_frame(const float (&v)[15], const PannerOptRow& o) {
  using namespace panner_geom;
  const V3 sp{v[0], v[1], v[2]}, so{v[3], v[4], v[5]}, lp{v[6], v[7], v[8]}, lf{v[9], v[10], v[11]}, lu{v[12], v[13], v[14]};
  // panner.rs:955-985 dist_gain (f64)
  float dg;
  {
    const double distance = (double)sqrtf(sqlen(sub(sp, lp)));
    const double ref = o.ref_distance, maxd = o.max_distance, roll = o.rolloff;
    double g;
    if (o.distance_model == 0) {  // linear
      const double rf = roll < 0. ? 0. : roll > 1. ? 1. : roll;
      const double lo = fmin(ref, maxd), hi = fmax(ref, maxd);
      const double dc = distance < lo ? lo : distance > hi ? hi : distance;
      g = 1. - rf * (dc - lo) / (hi - lo);
    } else if (o.distance_model == 1) {  // inverse
      const double rf = fmax(roll, 0.);
      g = distance > 0. ? ref / (ref + rf * (fmax(ref, distance) - ref)) : 1.;
    } else {
      const double rf = fmax(roll, 0.);
      g = pow(fmax(distance, ref) / ref, -rf);
    }
    dg = (float)g;
  }
  // panner.rs:927-953 cone_gain
  float cg;
  {
    const float in = fabsf(o.cone_inner) / 2.f, out = fabsf(o.cone_outer) / 2.f;
    if (in >= 180.f && out >= 180.f) {
      cg = 1.f;
    } else {
      const float a = spatial_angle(sp, so, lp);
      if (a < in)
        cg = 1.f;
      else if (a >= out)
        cg = o.cone_outer_gain;
      else {
        const float x = (a - in) / (out - in);
        cg = (1.f - x) + o.cone_outer_gain * x;
      }
    }
  }
  float a;
  azimuth_elevation(sp, lp, lf, lu, &a);
  // panner.rs:996-1004 wrap to [-90, 90]
  a = a < -180.f ? -180.f : a > 180.f ? 180.f : a;
  if (a < -90.f)
    a = -180.f - a;
  else if (a > 90.f)
    a = 180.f - a;
  const float xm = (a + 90.f) / 180.f;                                  // mono law, panner.rs:1006-1009
  const float xs = a <= 0.f ? (a + 90.f) / 90.f : a / 90.f;             // stereo law, panner.rs:1030-1040
  return {a, cosf(xm * PI_F / 2.f), sinf(xm * PI_F / 2.f), cosf(xs * PI_F / 2.f), sinf(xs * PI_F / 2.f), dg, cg};
}

}  // namespace waa

#endif  // WAA_PANNER_GEOM_HPP
