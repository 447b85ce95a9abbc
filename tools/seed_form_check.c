/* seed_form_check.c -- evidence for the closed-form FABRIK seed (seed_closed,
 * csrc/ik_fk_chain.h): FABRIK iteration counts with the seed pose computed as
 * J_k = Rz(theta_1) P_k, cos / sin(theta_1) = (x, y) / |(x, y)|, against the
 * oracle's restatement of the reference chain (inverse.py:123-130 -> fk_chain),
 * point by point, in float64 on the CPU.  Test infrastructure (includes the
 * oracle's C file); never part of the product.
 *
 *   gcc -O2 -fopenmp -ffp-contract=off -fno-builtin -o /tmp/seed_form_check  *       tools/seed_form_check.c -lm      (from the repo root)
 *   /tmp/seed_form_check N TOL MAX_ITER [0 random_dist-like | 1 uniform box]
 *
 * r06 (8 threads here): 10M points at 1e-3/100 and 1e-5/200, 2M uniform-box at
 * 1e-3/100, 2M at 1e-8/300: seeds differing in the last bits 89 %, iteration
 * mismatches 0 in every run.  (tol 0 is the exception by construction: there a
 * chain stops only on an exact fixed point, which any last-bit change moves.) */
#include "../oracle/ik_oracle.c"
#include <stdio.h>
#include <omp.h>

static void seed_closed(const double dh[16], pt3 g, pt3 J[4], const pt3 P[4]) {
  double r = sqrt(g.x * g.x + g.y * g.y);
  double c, s;
  if (r > 0 && isfinite(r)) { c = g.x / r; s = g.y / r; }
  else { double t = atan2(g.y, g.x); c = cos(t); s = sin(t); }
  for (int k = 0; k < 4; ++k) {
    J[k].x = c * P[k].x - s * P[k].y;
    J[k].y = s * P[k].x + c * P[k].y;
    J[k].z = P[k].z;
  }
}

int main(int argc, char **argv) {
  int64_t n = atoll(argv[1]);
  double tol = atof(argv[2]);
  int mi = atoi(argv[3]);
  int dist = argc > 4 ? atoi(argv[4]) : 0;
  double dh[16] = {0, IKO_PI / 2, 0, 0, 2, 0, 0, 0, 0, 2, 2, 2, IKO_PI / 2, 0, 0, 0};
  double links[4] = {2, 2, 2, 2};
  /* P_k: the chain at theta1 = 0 */
  double th0[4] = {0.0, dh[1], dh[2], dh[3]};
  pt3 P[4];
  fk_chain(dh, th0, P, 0);
  printf("P: %a %a %a | %a %a %a | %a %a %a | %a %a %a\n", P[0].x, P[0].y, P[0].z, P[1].x, P[1].y, P[1].z, P[2].x, P[2].y, P[2].z, P[3].x, P[3].y, P[3].z);
  int64_t bad = 0, badseed = 0, totit = 0;
  #pragma omp parallel for reduction(+:bad,badseed,totit) schedule(dynamic, 4096)
  for (int64_t i = 0; i < n; ++i) {
    /* splitmix64 -> points: normal(0, .5) truncated to the box (dist 0) or uniform box (1) */
    uint64_t z = (uint64_t)i * 0x9E3779B97F4A7C15ull + 12345;
    double v[3];
    for (int c = 0; c < 3; ++c) {
      static const double lo[3] = {0, -6, -3}, hi[3] = {6, 6, 6};
      for (;;) {
        z += 0x9E3779B97F4A7C15ull; uint64_t a = z; a = (a ^ (a >> 30)) * 0xBF58476D1CE4E5B9ull; a = (a ^ (a >> 27)) * 0x94D049BB133111EBull; a ^= a >> 31;
        z += 0x9E3779B97F4A7C15ull; uint64_t b = z; b = (b ^ (b >> 30)) * 0xBF58476D1CE4E5B9ull; b = (b ^ (b >> 27)) * 0x94D049BB133111EBull; b ^= b >> 31;
        double u1 = ((a >> 11) + 0.5) * 0x1p-53, u2 = ((b >> 11) + 0.5) * 0x1p-53;
        double x = dist ? lo[c] + (hi[c] - lo[c]) * u1 : 0.5 * sqrt(-2 * log(u1)) * cos(2 * IKO_PI * u2);
        if (x >= lo[c] && x <= hi[c]) { v[c] = x; break; }
      }
    }
    pt3 g = {v[0], v[1], v[2]};
    double th[4] = {atan2(g.y, g.x), dh[1], dh[2], dh[3]};
    pt3 cur[4], cur2[4], B[4], F[4];
    int st = fk_chain(dh, th, cur, 0), st2 = 0;
    seed_closed(dh, g, cur2, P);
    for (int k = 0; k < 4; ++k) if (cur[k].x != cur2[k].x || cur[k].y != cur2[k].y || cur[k].z != cur2[k].z) { badseed++; break; }
    int it = fabrik_calc(4, links, cur, g, tol, mi, &st, B, F);
    int it2 = fabrik_calc(4, links, cur2, g, tol, mi, &st2, B, F);
    totit += it;
    if (it != it2 || st != st2) bad++;
  }
  printf("n %lld tol %g mi %d dist %d: seeds differing %lld, iteration mismatches %lld, mean it %.3f\n",
         (long long)n, tol, mi, dist, (long long)badseed, (long long)bad, (double)totit / n);
  return 0;
}
