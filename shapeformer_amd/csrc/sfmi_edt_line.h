// One line of the separable squared distance transform (csrc/edt.hip): out[x] = min over y of f[y] + (x - y)^2 in
// integers, by the lower envelope of the parabolas (Meijster, Roerdink, Hesselink 2000, the second phase).  One caller walks one line;
// the line's elements are `stride` apart, so that the lanes of a wave, which walk neighbouring lines, touch consecutive addresses.
// Host and device: tests/test_voxfield_cpu.py compiles this file into a program that compares it with the double loop.
#pragma once

#ifndef __host__
#define __host__
#define __device__
#endif

// f[y] <= 2^28 + 2 * 513^2 and m <= 513: every intermediate below stays inside 32 bits
constexpr int SFMI_EDT_INF = 1 << 28;          // "no set voxel on the lines so far"; larger than any distance of a 513^3 lattice

__host__ __device__ inline int sfmi_edt_floordiv(int a, int b) {          // b > 0
  const int q = a / b;
  return (a % b != 0 && a < 0) ? q - 1 : q;
}

// f, out: m elements, `stride` apart; out must not be f.  S, T: m uint16 slots each, `stride` apart (the envelope's parabolas: where each
// stands and from where it is the lowest).  The top of the stack is kept in registers.
template <typename I16>
__host__ __device__ inline void sfmi_edt_line(const int* f, int* out, I16* S, I16* T, int m, int stride) {
  int q = 0, sq = 0, tq = 0, fq = f[0];
  S[0] = (I16)0;
  T[0] = (I16)0;
  for (int u = 1; u < m; ++u) {
    const int fu = f[u * stride];
    while (q >= 0 && (tq - sq) * (tq - sq) + fq > (tq - u) * (tq - u) + fu) {
      --q;
      if (q >= 0) {
        sq = (int)S[q * stride];
        tq = (int)T[q * stride];
        fq = f[sq * stride];
      }
    }
    if (q < 0) {
      q = 0; sq = u; tq = 0; fq = fu;
      S[0] = (I16)u;
    } else {
      // the first x at which parabola u is not above parabola sq
      const int w = 1 + sfmi_edt_floordiv(u * u - sq * sq + fu - fq, 2 * (u - sq));
      if (w < m) {
        ++q; sq = u; tq = w; fq = fu;
        S[q * stride] = (I16)u;
        T[q * stride] = (I16)w;
      }
    }
  }
  for (int u = m - 1; u >= 0; --u) {
    out[u * stride] = (u - sq) * (u - sq) + fq;
    if (u == tq) {
      --q;
      if (q >= 0) {
        sq = (int)S[q * stride];
        tq = (int)T[q * stride];
        fq = f[sq * stride];
      }
    }
  }
}
