// The face routines of the mesh queries, shared by csrc/meshsdf.hip (brute force) and csrc/meshtree.hip (the hierarchical route) so
// that both run the same instructions on a face: the closest point of a packed face record, the half solid angle of a triangle, and
// the packing of a face into its record with the degenerate-face rule.  Everything here is inlined into its caller and compiled under
// the build's contraction setting (an includer's `#pragma clang fp contract(off)` comes after this include), so a face gets the same
// bits in both files.  The lattice of the occupancy forms is here for the same reason.
//   record (5 x float4):  r0 = (a, |ab|^2)   r1 = (ab, ab.ac)   r2 = (ac, |ac|^2)   r3 = (b, wt)   r4 = (c, bad)
#pragma once
#include "sfmi_common.h"

constexpr int SFMI_FACE_REC = 5;                 // float4 per face record

__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
  return fmaf(az, bz, fmaf(ay, by, ax * bx));
}

// Closest point of the face record (a, ab, ac, d00 = ab.ab, d01 = ab.ac, d11 = ac.ac) to q as C = a + v ab + w ac; returns
// d2 = |q - C|^2 in the direct form.  Ericson's regions as selects, lowest priority first so that the first region of
// Ericson's order that holds is the one that stays.
__device__ __forceinline__ float closest_vw(float qx, float qy, float qz, const float4 r0, const float4 r1, const float4 r2, float& v,
                                            float& w) {
  const float apx = qx - r0.x, apy = qy - r0.y, apz = qz - r0.z;
  const float d1 = dot3(r1.x, r1.y, r1.z, apx, apy, apz);     // ab.ap
  const float d2 = dot3(r2.x, r2.y, r2.z, apx, apy, apz);     // ac.ap
  const float d3 = d1 - r0.w, d4 = d2 - r1.w;                 // ab.bp, ac.bp
  const float d5 = d1 - r1.w, d6 = d2 - r2.w;                 // ab.cp, ac.cp
  const float vc = fmaf(d1, d4, -(d3 * d2));
  const float vb = fmaf(d5, d2, -(d1 * d6));
  const float va = fmaf(d3, d6, -(d5 * d4));
  const float e43 = d4 - d3, e56 = d5 - d6;
  float nv = vb, nw = vc, den = va + vb + vc;                 // interior
  const bool rbc = va <= 0.f && e43 >= 0.f && e56 >= 0.f;     // edge BC: w' = e43 / (e43 + e56) along b -> c
  nv = rbc ? e56 : nv; nw = rbc ? e43 : nw; den = rbc ? e43 + e56 : den;
  const bool rac = vb <= 0.f && d2 >= 0.f && d6 <= 0.f;       // edge AC
  nv = rac ? 0.f : nv; nw = rac ? d2 : nw; den = rac ? d2 - d6 : den;
  const bool rc = d6 >= 0.f && d5 <= d6;                      // vertex C
  nv = rc ? 0.f : nv; nw = rc ? 1.f : nw; den = rc ? 1.f : den;
  const bool rab = vc <= 0.f && d1 >= 0.f && d3 <= 0.f;       // edge AB
  nv = rab ? d1 : nv; nw = rab ? 0.f : nw; den = rab ? d1 - d3 : den;
  const bool rb = d3 >= 0.f && d4 <= d3;                      // vertex B
  nv = rb ? 1.f : nv; nw = rb ? 0.f : nw; den = rb ? 1.f : den;
  const bool ra = d1 <= 0.f && d2 <= 0.f;                     // vertex A
  nv = ra ? 0.f : nv; nw = ra ? 0.f : nw; den = ra ? 1.f : den;
  const float rcp = den > 0.f ? __builtin_amdgcn_rcpf(den) : 0.f;
  v = nv * rcp;
  w = nw * rcp;
  const float cx = fmaf(w, r2.x, fmaf(v, r1.x, r0.x)), cy = fmaf(w, r2.y, fmaf(v, r1.y, r0.y)), cz = fmaf(w, r2.z, fmaf(v, r1.z, r0.z));
  const float dx = qx - cx, dy = qy - cy, dz = qz - cz;
  return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

// Omega / 2 of triangle (a, b, c) seen from q (van Oosterom-Strackee); finite for finite inputs (atan2(0, 0) = 0)
__device__ __forceinline__ float half_solid_angle(float qx, float qy, float qz, const float4 a, const float4 b, const float4 c) {
  const float ax = a.x - qx, ay = a.y - qy, az = a.z - qz;
  const float bx = b.x - qx, by = b.y - qy, bz = b.z - qz;
  const float cx = c.x - qx, cy = c.y - qy, cz = c.z - qz;
  const float la = sqrtf(dot3(ax, ay, az, ax, ay, az)), lb = sqrtf(dot3(bx, by, bz, bx, by, bz)),
              lc = sqrtf(dot3(cx, cy, cz, cx, cy, cz));
  const float kx = fmaf(by, cz, -(bz * cy)), ky = fmaf(bz, cx, -(bx * cz)), kz = fmaf(bx, cy, -(by * cx));
  const float det = dot3(ax, ay, az, kx, ky, kz);
  const float den = fmaf(dot3(cx, cy, cz, ax, ay, az), lb,
                         fmaf(dot3(bx, by, bz, cx, cy, cz), la, fmaf(dot3(ax, ay, az, bx, by, bz), lc, la * lb * lc)));
  return atan2f(det, den);
}

// The record of the face with vertices p[0], p[1], p[2] (all finite indices in range).  A degenerate face (zero area: repeated vertex,
// collinear vertices, or a width below 2^-22 of its longest edge) is stored as the segment of its longest edge, (P, Q-P, 0), for which
// closest_vw yields exactly the closest point of the segment (or of the point when P == Q), and with wt = 0: it adds nothing to the
// winding number.
__device__ __forceinline__ void sfmi_pack_face(const float (&p)[3][3], float4* __restrict__ r) {
  // degeneracy in f64 (the f32 inputs' products are exact there): width = |ab x ac| / longest edge <= 2^-22 longest edge
  double e[3][3], l2[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int k1 = (k + 1) % 3;
#pragma unroll
    for (int a = 0; a < 3; ++a) e[k][a] = (double)p[k1][a] - (double)p[k][a];     // edge k: vertex k -> vertex k+1
    l2[k] = e[k][0] * e[k][0] + e[k][1] * e[k][1] + e[k][2] * e[k][2];
  }
  const double ux = e[0][1] * -e[2][2] - e[0][2] * -e[2][1], uy = e[0][2] * -e[2][0] - e[0][0] * -e[2][2],
               uz = e[0][0] * -e[2][1] - e[0][1] * -e[2][0];                       // ab x ac (ac = -edge 2)
  const double cr2 = ux * ux + uy * uy + uz * uz;
  int km = 0;
  if (l2[1] > l2[km]) km = 1;
  if (l2[2] > l2[km]) km = 2;
  const double lmax2 = l2[km];
  const bool degen = cr2 <= 0x1.0p-44 * lmax2 * lmax2;
  float ax, ay, az, bx, by, bz, cx, cy, cz;                    // the record's a, ab, ac
  if (degen) {
    const int k1 = (km + 1) % 3;
    ax = p[km][0]; ay = p[km][1]; az = p[km][2];
    bx = p[k1][0] - ax; by = p[k1][1] - ay; bz = p[k1][2] - az;
    cx = cy = cz = 0.f;
  } else {
    ax = p[0][0]; ay = p[0][1]; az = p[0][2];
    bx = p[1][0] - ax; by = p[1][1] - ay; bz = p[1][2] - az;
    cx = p[2][0] - ax; cy = p[2][1] - ay; cz = p[2][2] - az;
  }
  r[0] = make_float4(ax, ay, az, dot3(bx, by, bz, bx, by, bz));
  r[1] = make_float4(bx, by, bz, dot3(bx, by, bz, cx, cy, cz));
  r[2] = make_float4(cx, cy, cz, dot3(cx, cy, cz, cx, cy, cz));
  r[3] = make_float4(p[1][0], p[1][1], p[1][2], degen ? 0.f : 1.f);
  r[4] = make_float4(p[2][0], p[2][1], p[2][2], 0.f);
}

// makeGrid 'on' mode coordinate: numpy linspace in f64 (i * step + lo, the last point exactly hi), then f32
struct Lattice {
  int G;
  double lo[3], hi[3], step[3];
};

__device__ __forceinline__ float lattice_coord(const Lattice& L, int a, long long i) {
  if (i == L.G - 1 && L.G > 1) return (float)L.hi[a];
  return (float)__dadd_rn(__dmul_rn((double)i, L.step[a]), L.lo[a]);
}

// ---- the winding sum in 2^-29 fixed point ---------------------------------------------------------------------------------------
constexpr float SD_WSCALE = 0x1.0p29f;           // a run's sum x 2^29, rounded, is bits 1.. of the partial: 2^31 faces x pi stay below 2^63
constexpr float INV_2PI = 0.15915494309189535f;               // W = sum(Omega / 2) / (2 pi)

// One run of the winding sum ends: add it to the integer partial and start the next from zero.  Bit 0 of a partial is set, and
// stays set, once a run was not finite (a non-finite query); the sums themselves are even.
__device__ __forceinline__ void w_flush(float& run, long long& acc) {
  acc += __float2ll_rn(run * SD_WSCALE) << 1;
  acc |= (long long)!(fabsf(run) < 1e6f);
  run = 0.f;
}

// the partials of one query, added up: bad when any has bit 0 set
__device__ __forceinline__ void w_add(long long p, long long& sum, bool& bad) {
  bad |= (p & 1) != 0;
  sum += p & ~1ll;
}

__device__ __forceinline__ float w_value(long long sum, bool bad) {
  return bad ? __int_as_float(0x7FC00000) : (float)((double)sum * 0x1.0p-30);   // exact up to the one rounding to f32
}
