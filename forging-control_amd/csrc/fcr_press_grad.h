// fcr_press_grad.h — the adjoint (vector-Jacobian product) of the press's RK4 step, open loop and with the controller
// in the loop, with respect to the states, the commands and the controller and — in the *_press
// kernels — to the 28 parameters of each trajectory's press (§7.15). Forward: fcr_plant.h (forging_rhs, rk4_step) and
// fcr_closed_loop.h (loop_body); nothing there is touched, this file only reads them.
//
// One lane owns one trajectory, as in the forward. The forward stored x[:, t] (the record) and u[:, t]; the adjoint runs
// t = S-1 .. 0 with lambda = dL/dx_{t+1} in registers:
//   lambda += g_x[:, t+1];  (lambda, g_u_plant) = rk4_step_vjp(x_t, u_t, lambda);  [controller];  write g_u / dv
// and ends with g_x0 = lambda + g_x[:, 0].
//
// rk4_step_vjp recomputes: the entry state of every sub-step forward from the stored x_t (kept in registers for the
// reference's 4 sub-steps: 4 x 5 doubles; any other count: recomputed per sub-step, (substeps-1) substeps / 2 extra
// sub-steps per step, nothing indexed at run time so nothing goes to the private segment), then per sub-step in reverse
// the stage points X2, X3, X4 (k4 is not needed), then four rhs_vjp. With incoming lambda and dt the sub-step:
//   a4 = dt/6 lambda,             mu4 = J^T(X4) a4
//   a3 = dt/3 lambda + dt   mu4,  mu3 = J^T(X3) a3
//   a2 = dt/3 lambda + dt/2 mu3,  mu2 = J^T(X2) a2
//   a1 = dt/6 lambda + dt/2 mu2,  mu1 = J^T(X1) a1
//   lambda += mu1 + mu2 + mu3 + mu4,   g_u += sum_i f_u^T a_i
//
// rhs_vjp is the sparse Jacobian of forging_rhs written out by hand, with the forward's sub-expressions recomputed
// beside it (one evaluation costs about one right-hand side). CONVENTIONS where the derivative is singular:
//   * deformation force: differentiated only where y > 0 && yd > 0. At yd == 0 the forward takes the branch and gives
//     fd = 0, but d(e_dot^M3)/d e_dot is infinite there; the derivative is taken as 0, so a press at rest has finite
//     gradients.
//   * valve flow q = c z sign(a) sqrt(k |a|): at a == 0 both dq/da and dq/dz are 0; the branch is chosen by z >= 0, as in
//     the forward.
//   * friction: slope FT / 0.5 where |yd| <= 0.5, 0 elsewhere.
//   * smooth pressure floor: derivative 0.5 (1 + p / sqrt(p^2 + eps)).
// Controller (closed loop): the fp32 chain is recomputed from the stored record with loop_body's fmaf order, so the
// ReLU masks and the Hardtanh mask are the forward's own; the float casts are treated as the identity, ReLU'(0) = 0, the
// Hardtanh mask is 1 only for -1 < v < 1.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fcr_plant.h"

namespace fcr {
namespace press_grad {

using plant::kLiteral;

constexpr int kMaxHidden = 256;   // the closed loop's widest controller (closed_loop::kClMaxHidden, fcr_closed_loop.h)

// ---- gradients with respect to the press ----
// The adjoint also collects (df/dc)^T a over the coefficients c that forging_rhs reads through its policy, per lane and
// along the same reverse recursion: rhs_vjp adds each evaluation's term to a CoeffGrad, the a_i of substep_vjp being the
// weights the parameter terms need as well. After the last step derive_vjp applies the transpose of derive()'s Jacobian:
// 26 sums -> the 28 fields of the lane's row. NoCoeffGrad: nothing is collected and no code is added — the kernels
// instantiated with it are the kernels they were.
// The sums are the members of plant::Coeffs but for four that share one: fd enters m1t, log m0, log k and log w0 alike,
// so `fd` holds sum -c1 fd and derive_vjp divides it by m0, k and w0. The conventions are the state gradients' own: the
// deformation coefficients receive gradient only where y > 0 && yd > 0; the valve's (flow_c, two_over_rho, ps, pt) 0 at a
// zero pressure difference, ps and pt by the branch z >= 0; ft receives yd / 0.5 inside the knee and 1 outside.
struct NoCoeffGrad {};
struct CoeffGrad {
    double fd = 0.0, m2 = 0.0, m3 = 0.0, m4 = 0.0, two_mu = 0.0, b0 = 0.0, a = 0.0, h0 = 0.0;
    double ps = 0.0, pt = 0.0, flow_c = 0.0, two_over_rho = 0.0;
    double half_v1 = 0.0, half_v2 = 0.0, a1 = 0.0, a2 = 0.0;
    double ft = 0.0, press1 = 0.0, press2 = 0.0, b_damp = 0.0, inv_m = 0.0, g = 0.0;
    double kb = 0.0, kl_1 = 0.0, kl_2 = 0.0, inv_t1 = 0.0;
};
template <class G>
constexpr bool kCollects = false;
template <>
inline constexpr bool kCollects<CoeffGrad> = true;

// gx += J_x(x, u)^T a, gu += f_u^T a (u does not enter the Jacobian: f4 = (u - z) / T1 is linear); G = CoeffGrad:
// gc += (df/dc)^T a.
template <bool SMOOTH, class P, class G>
__device__ __forceinline__ void rhs_vjp(const double (&x)[5], double u, const double (&a)[5], double (&gx)[5], double &gu,
                                        P p, G &gc) {
    const double y = x[0], yd = x[1], z = x[4];
    double p1 = x[2], p2 = x[3], d1 = 1.0, d2 = 1.0;          // effective pressures and their slopes
    if (SMOOTH) {
        const double r1 = sqrt(p1 * p1 + plant::kSmoothEps), r2 = sqrt(p2 * p2 + plant::kSmoothEps);
        d1 = 0.5 * (1.0 + p1 / r1);
        d2 = 0.5 * (1.0 + p2 / r2);
        p1 = 0.5 * (p1 + r1);
        p2 = 0.5 * (p2 + r2);
    }
    double fd_y = 0.0, fd_yd = 0.0;                             // d fd / d y, d fd / d yd
    [[maybe_unused]] double fd_on = 0.0;                        // fd itself (collecting only)
    if (y > 0.0 && yd > 0.0) {
        const double rh = 1.0 / (p.h0 - y);                     // 1/h1, d/dy = rh^2
        const double r = p.h0 * rh;                             // d/dy = r rh
        const double e = log(r);                                // d/dy = rh
        const double ra = exp(p.a * e);                         // d/dy = a ra rh
        const double w1 = p.w0 * ra;
        const double rr = r / ra;                               // d/dy = rr rh (1 - a)
        const double b1 = p.b0 * (1.0 + 0.67 * (rr - 1.0));
        const double db1 = p.b0 * 0.67 * rr * rh * (1.0 - p.a);
        const double num = p.two_mu * b1 * b1 + y * y, den = 4.0 * y * b1;
        const double kd = p.k * (1.0 + num / den);
        const double dnum = 2.0 * (p.two_mu * b1 * db1 + y), dden = 4.0 * (b1 + y * db1);
        const double dkd = p.k * (dnum * den - num * dden) / (den * den);
        const double ed = yd * rh;                              // log ed: d/dy = rh, d/dyd = 1/yd
        const double fd = kd * (w1 * b1) * p.m0 * exp(p.m1t + p.m2 * log(e) + p.m3 * log(ed) + p.m4 / e);
        fd_y = fd * (dkd / kd + p.a * rh + db1 / b1 + rh * (p.m2 / e + p.m3 - p.m4 / (e * e)));
        fd_yd = fd * p.m3 / yd;
        if constexpr (kCollects<G>) {
            // log fd = log kd + log w0 + a e + log b1 + log m0 + m1t + m2 log e + m3 log ed + m4 / e, kd = k (1 + num/den)
            fd_on = fd;
            const double w = -(a[1] * p.inv_m) * fd;
            const double ie = 1.0 / e;
            const double ikd = p.k / (den * kd);                // d log kd / d two_mu = ikd b1^2
            const double lb1 = 1.0 + ikd * (2.0 * p.two_mu * b1 * b1 - num);   // b1 d log fd / d b1
            const double t67 = lb1 * (p.b0 * 0.67 * rr / b1);   // rr d log fd / d rr (through b1)
            gc.fd += w;
            gc.m2 += w * log(e);
            gc.m3 += w * log(ed);
            gc.m4 += w * ie;
            gc.two_mu += w * ikd * b1 * b1;
            gc.b0 += w * lb1 / p.b0;                            // b1 is proportional to b0
            gc.a += w * e * (1.0 - t67);                        // ra = exp(a e); rr = r / ra
            // h0: d e / d h0 = -y rh / h0 (through r = h0 rh), d log ed / d h0 = -rh, rr = r^(1 - a)
            gc.h0 += w * (-y * rh / p.h0 * (p.a + ie * (p.m2 - p.m4 * ie) + t67 * (1.0 - p.a)) - p.m3 * rh);
        }
    }
    const bool work = z >= 0.0;
    const double apb = work ? p.ps - p1 : p1 - p.pt;
    const double aat = work ? p2 - p.pt : p.ps - p2;
    const double spb = sqrt(p.two_over_rho * fabs(apb)), sat = sqrt(p.two_over_rho * fabs(aat));
    const double qpb_z = p.flow_c * copysign(spb, apb), qat_z = p.flow_c * copysign(sat, aat);   // dq/dz (0 at a == 0)
    const double qpb_a = apb != 0.0 ? p.flow_c * z * p.two_over_rho / (2.0 * spb) : 0.0;        // dq/da
    const double qat_a = aat != 0.0 ? p.flow_c * z * p.two_over_rho / (2.0 * sat) : 0.0;
    const double qpb_p = work ? -qpb_a : qpb_a;                // d qpb / d p1_eff
    const double qat_p = work ? qat_a : -qat_a;                // d qat / d p2_eff
    const double v1 = p.half_v1 + p.a1 * y, v2 = p.half_v2 - p.a2 * y;
    const double in2 = qpb_z * z * (1.0 / 3.0) - p.a1 * yd - p.kl_1 * p1;    // f2 = kb / v1 * in2
    const double in3 = -0.5 * (qat_z * z) + p.a2 * yd - p.kl_2 * p2;         // f3 = kb / v2 * in3
    const double ft_s = fabs(yd) <= 0.5 ? p.ft / 0.5 : 0.0;
    const double c1 = a[1] * p.inv_m, c2 = a[2] * (p.kb / v1), c3 = a[3] * (p.kb / v2);
    gx[0] += -c1 * fd_y - c2 * in2 * (p.a1 / v1) + c3 * in3 * (p.a2 / v2);
    gx[1] += a[0] - c1 * (p.b_damp + ft_s + fd_yd) - c2 * p.a1 + c3 * p.a2;
    gx[2] += d1 * (c1 * p.press1 + c2 * (qpb_p * (1.0 / 3.0) - p.kl_1));
    gx[3] += d2 * (-c1 * p.press2 + c3 * (-0.5 * qat_p - p.kl_2));
    gx[4] += c2 * qpb_z * (1.0 / 3.0) - 0.5 * c3 * qat_z - a[4] * p.inv_t1;
    gu += a[4] * p.inv_t1;
    if constexpr (kCollects<G>) {
        const bool knee = fabs(yd) <= 0.5;
        const double s = p.press1 * p1 - p.press2 * p2 - p.b_damp * yd - (knee ? p.ft * yd / 0.5 : p.ft) - fd_on;
        gc.inv_m += a[1] * s;
        gc.g += a[1];
        gc.press1 += c1 * p1;
        gc.press2 -= c1 * p2;
        gc.b_damp -= c1 * yd;
        gc.ft -= c1 * (knee ? yd / 0.5 : 1.0);
        const double i2 = in2 / v1, i3 = in3 / v2;
        gc.kb += a[2] * i2 + a[3] * i3;
        gc.half_v1 -= c2 * i2;
        gc.half_v2 -= c3 * i3;
        gc.a1 -= c2 * (i2 * y + yd);
        gc.a2 += c3 * (i3 * y + yd);
        gc.kl_1 -= c2 * p1;
        gc.kl_2 -= c3 * p2;
        gc.inv_t1 += a[4] * (u - z);
        const double wpb = c2 * (1.0 / 3.0), wat = -0.5 * c3;  // dL / d qpb, dL / d qat
        gc.flow_c += (wpb * copysign(spb, apb) + wat * copysign(sat, aat)) * z;           // q / flow_c
        gc.two_over_rho += (wpb * qpb_z + wat * qat_z) * z / (2.0 * p.two_over_rho);       // q / (2 two_over_rho)
        const double dpb = wpb * qpb_a, dat = wat * qat_a;     // dL / d apb, dL / d aat (0 at a zero difference)
        gc.ps += work ? dpb : dat;                             // apb = ps - p1, aat = p2 - pt | apb = p1 - pt, aat = ps - p2
        gc.pt -= work ? dat : dpb;
    }
}

// The transpose of derive()'s Jacobian at `row`: the lane's sums -> the gradient of its 28 fields (fcr_press's order).
__device__ __forceinline__ void derive_vjp(const double *row, const CoeffGrad &gc, double (&g)[plant::kPressFields]) {
    const double m_mass = row[0], d1 = row[3], d2 = row[4], cd = row[11], rho = row[12], d = row[13];
    const double k = row[17], w0 = row[18], b0 = row[20], t_def = row[21], t1 = row[22], m0 = row[23], m1 = row[24];
    const double s = b0 / w0, da = 0.36 - 0.108 * s;           // a = 0.14 + 0.36 s - 0.054 s^2
    g[0] = -gc.inv_m / (m_mass * m_mass);
    g[1] = gc.b_damp;
    g[2] = gc.ft;
    g[3] = (gc.a1 / 4 + 3 * gc.press1 / 4) * 2 * plant::kPi * d1;
    g[4] = (gc.a2 / 4 + gc.press2 / 2) * 2 * plant::kPi * d2;
    g[5] = gc.g;
    g[6] = gc.kb;
    g[7] = gc.half_v1 / 2;
    g[8] = gc.half_v2 / 2;
    g[9] = gc.kl_1;
    g[10] = gc.kl_2;
    g[11] = gc.flow_c * plant::kPi * d;
    g[12] = -2.0 * gc.two_over_rho / (rho * rho);
    g[13] = gc.flow_c * plant::kPi * cd;
    g[14] = gc.ps;
    g[15] = gc.pt;
    g[16] = 2.0 * gc.two_mu;
    g[17] = gc.fd / k;
    g[18] = gc.fd / w0 - gc.a * da * s / w0;
    g[19] = gc.h0;
    g[20] = gc.b0 + gc.a * da / w0;
    g[21] = gc.fd * m1;
    g[22] = -gc.inv_t1 / (t1 * t1);
    g[23] = gc.fd / m0;
    g[24] = gc.fd * t_def;
    g[25] = gc.m2;
    g[26] = gc.m3;
    g[27] = gc.m4;
}

// The adjoint of ONE RK4 sub-step entered at x: lam (dL/d x_out) -> dL/d x, gu += dL/du, gc += dL/dc.
template <bool SMOOTH, class P, class G>
__device__ __forceinline__ void substep_vjp(const double (&x)[5], double u, double dt, double (&lam)[5], double &gu, P p,
                                            G &gc) {
    double k[5], x2[5], x3[5], x4[5];
    plant::forging_rhs<SMOOTH>(x, u, k, p);
#pragma unroll
    for (int i = 0; i < 5; ++i) x2[i] = x[i] + dt / 2 * k[i];
    plant::forging_rhs<SMOOTH>(x2, u, k, p);
#pragma unroll
    for (int i = 0; i < 5; ++i) x3[i] = x[i] + dt / 2 * k[i];
    plant::forging_rhs<SMOOTH>(x3, u, k, p);
#pragma unroll
    for (int i = 0; i < 5; ++i) x4[i] = x[i] + dt * k[i];
    double a[5], mu[5], sum[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        a[i] = dt / 6 * lam[i];
        mu[i] = 0.0;
    }
    rhs_vjp<SMOOTH>(x4, u, a, mu, gu, p, gc);
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        sum[i] = mu[i];
        a[i] = dt / 3 * lam[i] + dt * mu[i];
        mu[i] = 0.0;
    }
    rhs_vjp<SMOOTH>(x3, u, a, mu, gu, p, gc);
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        sum[i] += mu[i];
        a[i] = dt / 3 * lam[i] + dt / 2 * mu[i];
        mu[i] = 0.0;
    }
    rhs_vjp<SMOOTH>(x2, u, a, mu, gu, p, gc);
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        sum[i] += mu[i];
        a[i] = dt / 6 * lam[i] + dt / 2 * mu[i];
        mu[i] = 0.0;
    }
    rhs_vjp<SMOOTH>(x, u, a, mu, gu, p, gc);
#pragma unroll
    for (int i = 0; i < 5; ++i) lam[i] += sum[i] + mu[i];
}

constexpr int kKeptSubsteps = 4;   // the reference's count: the sub-steps' entry states stay in registers

// The adjoint of one sampling step of `substeps` sub-steps from the stored xt under the held command u.
// KEPT: substeps == kKeptSubsteps, every loop unrolled; otherwise each sub-step's entry state is recomputed from xt.
template <bool SMOOTH, bool KEPT, class P, class G>
__device__ __forceinline__ void rk4_step_vjp(const double (&xt)[5], double u, double dt, int substeps, double (&lam)[5],
                                             double &gu, P p, G &gc) {
    if constexpr (KEPT) {
        // The entry states e1..e3 are named registers picked by compare-and-select, and both loops stay rolled: one
        // sub-step and one sub-step adjoint in the code. Unrolled (3 + 4 bodies of 4 right-hand sides each) the
        // compiler interleaves them, asks for all 512 registers and spills 0.4-1.3 KB per lane.
        double e1[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, e2[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, e3[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, e[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) e[i] = xt[i];
#pragma nounroll
        for (int m = 1; m < kKeptSubsteps; ++m) {
            plant::rk4_step<SMOOTH, false>(e, u, dt, 1, nullptr, p);
#pragma unroll
            for (int i = 0; i < 5; ++i) {
                e1[i] = m == 1 ? e[i] : e1[i];
                e2[i] = m == 2 ? e[i] : e2[i];
                e3[i] = m == 3 ? e[i] : e3[i];
            }
        }
#pragma nounroll
        for (int m = kKeptSubsteps - 1; m >= 0; --m) {
#pragma unroll
            for (int i = 0; i < 5; ++i) e[i] = m == 3 ? e3[i] : (m == 2 ? e2[i] : (m == 1 ? e1[i] : xt[i]));
            substep_vjp<SMOOTH>(e, u, dt, lam, gu, p, gc);
        }
    } else {
        for (int m = substeps - 1; m >= 0; --m) {
            double e[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) e[i] = xt[i];
            plant::rk4_step<SMOOTH, false>(e, u, dt, m, nullptr, p);
            substep_vjp<SMOOTH>(e, u, dt, lam, gu, p, gc);
        }
    }
}

// this lane's press: the reference's (P = Nominal) or row b * stride of a table (P = Coeffs)
template <class P>
__device__ __forceinline__ P lane_press(const double *press, long long stride, int b) {
    if constexpr (kLiteral<P>) return {};
    else return plant::derive(press + (size_t)b * stride);
}

constexpr int kGradBlock = 256;

// where a collecting lane leaves its row's gradient: g_press[b * 28 + i], after derive_vjp at the row derive() read
template <class G>
__device__ __forceinline__ void store_press_grad(const double *press, long long stride, int b, const G &gc,
                                                 double *__restrict__ g_press) {
    if constexpr (kCollects<G>) {
        double g[plant::kPressFields];
        derive_vjp(press + (size_t)b * stride, gc, g);
#pragma unroll
        for (int i = 0; i < plant::kPressFields; ++i) g_press[(size_t)b * plant::kPressFields + i] = g[i];
    }
}

// Open loop: x (B,S+1,5) and u (B,S) as fcr_plant_rk4 stored them, g_x (B,S+1,5) incoming -> g_x0 (B,5), g_u (B,S);
// G = CoeffGrad: and g_press (B,28), each trajectory's own whatever the table's stride.
template <bool SMOOTH, bool KEPT, class P, class G>
__device__ __forceinline__ void plant_rk4_vjp_body(int B, int S, double dt, int substeps, const double *__restrict__ x,
                                                   const double *__restrict__ u, const double *__restrict__ g_x,
                                                   const double *__restrict__ press, long long stride_traj,
                                                   double *__restrict__ g_x0, double *__restrict__ g_u,
                                                   double *__restrict__ g_press) {
    const int b = blockIdx.x * kGradBlock + threadIdx.x;
    if (b >= B) return;
    const P p = lane_press<P>(press, stride_traj, b);
    const double *xb = x + (size_t)b * (S + 1) * 5, *gb = g_x + (size_t)b * (S + 1) * 5, *ub = u + (size_t)b * S;
    double *go = g_u + (size_t)b * S;
    double lam[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    G gc;
    for (int t = S - 1; t >= 0; --t) {
        double xt[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            lam[i] += gb[(size_t)(t + 1) * 5 + i];
            xt[i] = xb[(size_t)t * 5 + i];
        }
        double gu = 0.0;
        rk4_step_vjp<SMOOTH, KEPT>(xt, ub[t], dt, substeps, lam, gu, p, gc);
        go[t] = gu;
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) g_x0[(size_t)b * 5 + i] = lam[i] + gb[i];
    store_press_grad(press, stride_traj, b, gc, g_press);
}

template <bool SMOOTH, bool KEPT, class P>
__global__ __launch_bounds__(kGradBlock) void plant_rk4_vjp_kernel(int B, int S, double dt, int substeps,
                                                                   const double *__restrict__ x,
                                                                   const double *__restrict__ u,
                                                                   const double *__restrict__ g_x,
                                                                   const double *__restrict__ press, long long stride_traj,
                                                                   double *__restrict__ g_x0, double *__restrict__ g_u) {
    plant_rk4_vjp_body<SMOOTH, KEPT, P, NoCoeffGrad>(B, S, dt, substeps, x, u, g_x, press, stride_traj, g_x0, g_u, nullptr);
}

// ... with the gradient of every trajectory's press (a table's rows only: the reference's literals have none)
template <bool SMOOTH, bool KEPT>
__global__ __launch_bounds__(kGradBlock) void plant_rk4_vjp_press_kernel(int B, int S, double dt, int substeps,
                                                                         const double *__restrict__ x,
                                                                         const double *__restrict__ u,
                                                                         const double *__restrict__ g_x,
                                                                         const double *__restrict__ press,
                                                                         long long stride_traj, double *__restrict__ g_x0,
                                                                         double *__restrict__ g_u,
                                                                         double *__restrict__ g_press) {
    plant_rk4_vjp_body<SMOOTH, KEPT, plant::Coeffs, CoeffGrad>(B, S, dt, substeps, x, u, g_x, press, stride_traj, g_x0, g_u,
                                                               g_press);
}

struct LoopGradArgs {
    int B, T, substeps, hidden;
    double dt;
    const double *ref;
    const float *w_inp, *b_inp, *w_out;
    double in_scale0, in_scale1, ref_scale, out_scale;
    const double *x, *u, *g_x, *g_u;      // the stored run; the incoming gradients
    const double *press;                  // P = Coeffs: the table
    long long stride_traj;
    double *g_x0, *dv;
};

// Closed loop: the same recursion with the controller in it. Per step, after the plant's adjoint at the stored
// (x_t, u_t): du = g_u[b,t] + (plant's g_u); the fp32 chain is recomputed from the record as loop_body evaluates it;
// dv = du * out_scale * [-1 < v < 1]; dz_j = dv * w_out[j] * [z_j > 0]; lambda[1] += sum_j dz_j w_inp[j][0] / in_scale0,
// lambda[4] += sum_j dz_j w_inp[j][1] / in_scale1; dv[b,t] is written for the parameter gradients' kernel below.
template <bool SMOOTH, bool KEPT, class P>
__global__ __launch_bounds__(kGradBlock) void closed_loop_vjp_kernel(LoopGradArgs a) {
    __shared__ float w[kMaxHidden * 5];        // [j] = (w_inp[j][0..2], b_inp[j], w_out[j]), as loop_body
    for (int i = threadIdx.x; i < a.hidden; i += kGradBlock) {
        w[i * 5 + 0] = a.w_inp[i * 3 + 0];
        w[i * 5 + 1] = a.w_inp[i * 3 + 1];
        w[i * 5 + 2] = a.w_inp[i * 3 + 2];
        w[i * 5 + 3] = a.b_inp[i];
        w[i * 5 + 4] = a.w_out[i];
    }
    __syncthreads();
    const int b = blockIdx.x * kGradBlock + threadIdx.x;
    if (b >= a.B) return;
    const P p = lane_press<P>(a.press, a.stride_traj, b);
    const size_t row = (size_t)b * a.T;
    const double *xb = a.x + (size_t)b * (a.T + 1) * 5, *gb = a.g_x + (size_t)b * (a.T + 1) * 5;
    const double os = (double)(float)a.out_scale;             // the forward multiplies by the float32 scale
    double lam[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    NoCoeffGrad gc;
    for (int t = a.T - 1; t >= 0; --t) {
        double xt[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            lam[i] += gb[(size_t)(t + 1) * 5 + i];
            xt[i] = xb[(size_t)t * 5 + i];
        }
        double du = a.g_u[row + t];
        rk4_step_vjp<SMOOTH, KEPT>(xt, a.u[row + t], a.dt, a.substeps, lam, du, p, gc);
        const float s0 = (float)(xt[1] / a.in_scale0), s1 = (float)(xt[4] / a.in_scale1);
        const float s2 = (float)(a.ref[row + t] / a.ref_scale);
        float v = 0.0f;
        for (int j = 0; j < a.hidden; ++j) {
            const float *wj = w + j * 5;
            float z = fmaf(wj[2], s2, fmaf(wj[1], s1, fmaf(wj[0], s0, wj[3])));
            z = z > 0.0f ? z : 0.0f;
            v = fmaf(wj[4], z, v);
        }
        const double dv = (v > -1.0f && v < 1.0f) ? du * os : 0.0;
        a.dv[row + t] = dv;
        if (dv != 0.0) {
            double g0 = 0.0, g1 = 0.0;
            for (int j = 0; j < a.hidden; ++j) {
                const float *wj = w + j * 5;
                const float z = fmaf(wj[2], s2, fmaf(wj[1], s1, fmaf(wj[0], s0, wj[3])));
                if (z > 0.0f) {
                    const double dz = dv * (double)wj[4];
                    g0 = fma(dz, (double)wj[0], g0);
                    g1 = fma(dz, (double)wj[1], g1);
                }
            }
            lam[1] += g0 / a.in_scale0;
            lam[4] += g1 / a.in_scale1;
        }
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) a.g_x0[(size_t)b * 5 + i] = lam[i] + gb[i];
}

// (The body is repeated, not shared: called from one __device__ function taking the collector, closed_loop_vjp_kernel
// comes out with its prologue rescheduled — the same work, but no longer the parent's instructions, as fcr_plant.h found
// for plant_rk4_kernel. The open loop's kernels above do share theirs: they come out as they were.)
// closed_loop_vjp_kernel with the gradient of every trajectory's press: g_press (B,28), a table's rows only.
template <bool SMOOTH, bool KEPT>
__global__ __launch_bounds__(kGradBlock) void closed_loop_vjp_press_kernel(LoopGradArgs a, double *__restrict__ g_press) {
    __shared__ float w[kMaxHidden * 5];        // [j] = (w_inp[j][0..2], b_inp[j], w_out[j]), as loop_body
    for (int i = threadIdx.x; i < a.hidden; i += kGradBlock) {
        w[i * 5 + 0] = a.w_inp[i * 3 + 0];
        w[i * 5 + 1] = a.w_inp[i * 3 + 1];
        w[i * 5 + 2] = a.w_inp[i * 3 + 2];
        w[i * 5 + 3] = a.b_inp[i];
        w[i * 5 + 4] = a.w_out[i];
    }
    __syncthreads();
    const int b = blockIdx.x * kGradBlock + threadIdx.x;
    if (b >= a.B) return;
    const plant::Coeffs p = lane_press<plant::Coeffs>(a.press, a.stride_traj, b);
    const size_t row = (size_t)b * a.T;
    const double *xb = a.x + (size_t)b * (a.T + 1) * 5, *gb = a.g_x + (size_t)b * (a.T + 1) * 5;
    const double os = (double)(float)a.out_scale;             // the forward multiplies by the float32 scale
    double lam[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    CoeffGrad gc;
    for (int t = a.T - 1; t >= 0; --t) {
        double xt[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            lam[i] += gb[(size_t)(t + 1) * 5 + i];
            xt[i] = xb[(size_t)t * 5 + i];
        }
        double du = a.g_u[row + t];
        rk4_step_vjp<SMOOTH, KEPT>(xt, a.u[row + t], a.dt, a.substeps, lam, du, p, gc);
        const float s0 = (float)(xt[1] / a.in_scale0), s1 = (float)(xt[4] / a.in_scale1);
        const float s2 = (float)(a.ref[row + t] / a.ref_scale);
        float v = 0.0f;
        for (int j = 0; j < a.hidden; ++j) {
            const float *wj = w + j * 5;
            float z = fmaf(wj[2], s2, fmaf(wj[1], s1, fmaf(wj[0], s0, wj[3])));
            z = z > 0.0f ? z : 0.0f;
            v = fmaf(wj[4], z, v);
        }
        const double dv = (v > -1.0f && v < 1.0f) ? du * os : 0.0;
        a.dv[row + t] = dv;
        if (dv != 0.0) {
            double g0 = 0.0, g1 = 0.0;
            for (int j = 0; j < a.hidden; ++j) {
                const float *wj = w + j * 5;
                const float z = fmaf(wj[2], s2, fmaf(wj[1], s1, fmaf(wj[0], s0, wj[3])));
                if (z > 0.0f) {
                    const double dz = dv * (double)wj[4];
                    g0 = fma(dz, (double)wj[0], g0);
                    g1 = fma(dz, (double)wj[1], g1);
                }
            }
            lam[1] += g0 / a.in_scale0;
            lam[4] += g1 / a.in_scale1;
        }
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) a.g_x0[(size_t)b * 5 + i] = lam[i] + gb[i];
    store_press_grad(a.press, a.stride_traj, b, gc, g_press);
}

// A shared press (one row, stride 0) receives the sum over the trajectories of g_press (B,28), in fp64 and in a fixed
// order, as the controller's parameters below: block k adds the trajectories 256 k .. 256 k + 255 in order, lane i its
// column i, into part[k][28]; press_grad_reduce_kernel adds the blocks in order. The grid is a function of B alone.
constexpr int kSumLanes = 64;   // one wave; 28 of its lanes work

__global__ __launch_bounds__(kSumLanes) void press_grad_sum_kernel(int B, const double *__restrict__ g_press,
                                                                   double *__restrict__ part) {
    const int i = threadIdx.x;
    if (i >= plant::kPressFields) return;
    const long long first = (long long)blockIdx.x * kGradBlock;
    const long long last = first + kGradBlock < B ? first + kGradBlock : B;
    double sum = 0.0;
    for (long long b = first; b < last; ++b) sum += g_press[(size_t)b * plant::kPressFields + i];
    part[(size_t)blockIdx.x * plant::kPressFields + i] = sum;
}

// g_row (28) = the blocks' partials added in block order; blocks = 0: zeros.
__global__ __launch_bounds__(kSumLanes) void press_grad_reduce_kernel(const double *__restrict__ part, int blocks,
                                                                      double *__restrict__ g_row) {
    const int i = threadIdx.x;
    if (i >= plant::kPressFields) return;
    double sum = 0.0;
    for (int q = 0; q < blocks; ++q) sum += part[(size_t)q * plant::kPressFields + i];
    g_row[i] = sum;
}

// The controller's parameter gradients from dv: sums over all rows (b,t) of dv relu_j (g_w_out), dz_j s_k (g_w_inp) and
// dz_j (g_b_inp), in fp64 and in a fixed order — no atomics, so two runs give the same bits. Block k takes the tiles
// k, k + gridDim.x, ... of 256 rows; a tile's (s0, s1, s2, dv) is staged in LDS; lane (g, j) = (tid / H, tid % H) owns
// unit j and adds the tile's rows g, g + groups, ... (groups = 256 / H) to five sums in its registers, z_j recomputed from
// the record with the forward's fmaf order. Then the groups are added in order and block k writes part[k][j][5];
// param_reduce_kernel adds the blocks in order. The grid is a function of (B, T) alone (param_blocks).
constexpr int kParamMaxBlocks = 512;

__host__ __device__ inline int param_blocks(long long rows) {
    const long long tiles = (rows + kGradBlock - 1) / kGradBlock;
    return (int)(tiles < kParamMaxBlocks ? tiles : kParamMaxBlocks);
}

__global__ __launch_bounds__(kGradBlock) void param_grad_kernel(LoopGradArgs a, double *__restrict__ part) {
    __shared__ float s0[kGradBlock], s1[kGradBlock], s2[kGradBlock];
    __shared__ double dvs[kGradBlock];
    __shared__ double red[kGradBlock * 5];
    const int tid = threadIdx.x, H = a.hidden, groups = kGradBlock / H;
    const int g = tid / H, j = tid - g * H;
    const bool on = g < groups;
    float w0 = 0.0f, w1 = 0.0f, w2 = 0.0f, bj = 0.0f, wo = 0.0f;
    if (on) {
        w0 = a.w_inp[j * 3 + 0], w1 = a.w_inp[j * 3 + 1], w2 = a.w_inp[j * 3 + 2];
        bj = a.b_inp[j], wo = a.w_out[j];
    }
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const long long rows = (long long)a.B * a.T, tiles = (rows + kGradBlock - 1) / kGradBlock;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const long long r = tile * kGradBlock + tid;
        __syncthreads();                                       // the previous tile has been read
        if (r < rows) {
            const long long b = r / a.T, t = r - b * a.T;
            const double *xr = a.x + (size_t)(b * (a.T + 1) + t) * 5;
            s0[tid] = (float)(xr[1] / a.in_scale0);
            s1[tid] = (float)(xr[4] / a.in_scale1);
            s2[tid] = (float)(a.ref[r] / a.ref_scale);
            dvs[tid] = a.dv[r];
        } else {
            s0[tid] = s1[tid] = s2[tid] = 0.0f;
            dvs[tid] = 0.0;
        }
        __syncthreads();
        if (on) {
            for (int i = g; i < kGradBlock; i += groups) {
                const double d = dvs[i];
                if (d == 0.0) continue;                        // a saturated (or padding) row adds nothing
                const float z = fmaf(w2, s2[i], fmaf(w1, s1[i], fmaf(w0, s0[i], bj)));
                if (z > 0.0f) {
                    const double dz = d * (double)wo;
                    acc[0] = fma(dz, (double)s0[i], acc[0]);
                    acc[1] = fma(dz, (double)s1[i], acc[1]);
                    acc[2] = fma(dz, (double)s2[i], acc[2]);
                    acc[3] += dz;
                    acc[4] = fma(d, (double)z, acc[4]);
                }
            }
        }
    }
    __syncthreads();
    if (on) {
#pragma unroll
        for (int k = 0; k < 5; ++k) red[(size_t)tid * 5 + k] = acc[k];   // tid = g * H + j
    }
    __syncthreads();
    if (tid < H) {
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            double sum = 0.0;
            for (int q = 0; q < groups; ++q) sum += red[(size_t)(q * H + tid) * 5 + k];
            part[((size_t)blockIdx.x * H + tid) * 5 + k] = sum;
        }
    }
}

// g_w_inp (H,3), g_b_inp (H), g_w_out (H) = the blocks' partials added in block order; blocks = 0: zeros.
__global__ __launch_bounds__(kGradBlock) void param_reduce_kernel(const double *__restrict__ part, int blocks, int H,
                                                                  double *__restrict__ g_w_inp,
                                                                  double *__restrict__ g_b_inp,
                                                                  double *__restrict__ g_w_out) {
    const int idx = blockIdx.x * kGradBlock + threadIdx.x;
    if (idx >= H * 5) return;
    const int j = idx / 5, k = idx - j * 5;
    double sum = 0.0;
    for (int q = 0; q < blocks; ++q) sum += part[((size_t)q * H + j) * 5 + k];
    if (k < 3) g_w_inp[j * 3 + k] = sum;
    else if (k == 3) g_b_inp[j] = sum;
    else g_w_out[j] = sum;
}

}  // namespace press_grad
}  // namespace fcr
