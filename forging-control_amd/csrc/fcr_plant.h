// fcr_plant.h — the open-die forging press as a batched fp64 RK4 integrator.
//
// Reference: FeasibilityRecovery.forging_model (Functions.py:1615-1740) / template_model
// (template_model.py:19-149, pressures floored by smooth_relu, :106-118), integrated by
// FeasibilityRecovery.Ruge_Kuta (Functions.py:1743-1781): M = 4 RK4 sub-steps of TS/M with the command
// held, all in fp64 as CasADi's SX evaluation is.
//
// One lane owns one trajectory for the whole horizon: its 5 states stay in VGPRs across the S steps
// and 4·S right-hand sides; HBM sees the command (8 B) in and the state (40 B) out per step. Each
// right-hand side is ~500 fp64-path VALU instructions (3 logs, 2 exps, 2 square roots, 5 divisions, all
// software sequences; constant divisors are folded into reciprocal products) — the kernel is bound by
// VALU issue, not by HBM (48 B per 16 right-hand sides).
//
// The algebra of the deformation force is regrouped so one log of the height ratio feeds every power:
//   r = H0/h1, e = log r, r^A = exp(A e), H0/h1 · W0/w1 = r / r^A,
//   e^M2 · ė^M3 · exp(M1 T) · exp(M4/e) = exp(M1 T + M2 log e + M3 log ė + M4/e)
// (ė = 0 -> log ė = -inf -> exp(-inf) = 0 = 0^M3, as the reference); results agree with the literal
// restatement (oracle/plant_np.py) to a few ulp per step.
#pragma once
#include <hip/hip_runtime.h>

namespace fcr {
namespace plant {

constexpr double kPi = 3.14159265358979323846;
constexpr double M_MASS = 90000.0, B_DAMP = 25000.0, FT = 200000.0;   // Functions.py:1636-1643
constexpr double D1 = 0.6, D2 = 0.5, G = 9.81;
constexpr double A1 = kPi * D1 * D1 / 4, A2 = kPi * D2 * D2 / 4;
constexpr double KB = 22e9, V1_0 = 0.3, V2_0 = 0.1, KL_1 = 8e-13, KL_2 = 14e-14;   // :1646-1650
constexpr double CD = 0.63, RHO = 858.0, D = 0.006;                           // :1653-1655
constexpr double PS = 32e6, PT = 101325.0;                                    // :1660-1661
constexpr double MU = 0.3, K = 1.115, W0 = 0.2, H0 = 0.5, B0 = 0.1;          // :1664-1668
constexpr double A = 0.14 + 0.36 * (B0 / W0) - 0.054 * (B0 / W0) * (B0 / W0);   // :1671
constexpr double T_DEF = 900.0, T1 = 0.005;                                   // :1677, :1680
constexpr double M0 = 1200e6, M1 = -0.0025, M2 = -0.0587, M3 = 0.1165, M4 = -0.0065;   // :1691-1695
constexpr double kSmoothEps = 1e-6;                                           // template_model.py:113
constexpr double kFlowC = kPi * D * CD;                                       // q = kFlowC·z·sqrt(2|a|/RHO)·sign(a)
constexpr double kTwoOverRho = 2.0 / RHO;
constexpr double kPress1 = 3 * kPi * D1 * D1 / 4, kPress2 = kPi * D2 * D2 / 2;

// ---- the press and the workpiece as a parameter policy ----
// forging_rhs reads every machine constant through a policy P. Nominal: the constexpr values above, members of an empty
// struct, so every expression folds as it always did and the kernels instantiated with it are the kernels they were.
// Coeffs: the same coefficients as run-time doubles, formed once from a row of 28 parameters (fcr_press, include/fcr.h)
// by derive() below — per lane in VGPRs (the true plant of one trajectory: LaneParams) or per launch on the host and
// passed by value as a kernel argument, held in scalar registers (the model a projection integrates: UniformParams).
// The friction knee (0.5 m/s) and kSmoothEps are the model's form, not the machine, and stay constants.
struct Nominal {
    static constexpr double h0 = H0, a = A, w0 = W0, b0 = B0, k = K, two_mu = 2.0 * MU;
    static constexpr double m0 = M0, m1t = M1 * T_DEF, m2 = M2, m3 = M3, m4 = M4;
    static constexpr double ps = PS, pt = PT, flow_c = kFlowC, two_over_rho = kTwoOverRho;
    static constexpr double half_v1 = V1_0 / 2, half_v2 = V2_0 / 2, a1 = A1, a2 = A2;
    static constexpr double ft = FT, press1 = kPress1, press2 = kPress2, b_damp = B_DAMP, inv_m = 1.0 / M_MASS, g = G;
    static constexpr double kb = KB, kl_1 = KL_1, kl_2 = KL_2, inv_t1 = 1.0 / T1;
};

constexpr int kPressFields = 28;   // doubles per row of a parameter table: the fields of fcr_press, in its order

struct Coeffs {
    double h0, a, w0, b0, k, two_mu;                         // the deformation-force group: read under y > 0 && yd >= 0
    double m0, m1t, m2, m3, m4;
    double ps, pt, flow_c, two_over_rho;
    double half_v1, half_v2, a1, a2;
    double ft, press1, press2, b_damp, inv_m, g;
    double kb, kl_1, kl_2, inv_t1;
};
using LaneParams = Coeffs;      // one trajectory's own press, in that lane's registers
using UniformParams = Coeffs;   // one press for the whole launch, a kernel argument

// row = [m_mass, b_damp, ft, d1, d2, g, kb, v1_0, v2_0, kl_1, kl_2, cd, rho, d, ps, pt, mu, k, w0, h0, b0, t_def, t1,
// m0, m1, m2, m3, m4]. Every coefficient has the expression and the operation order of its constexpr above and nothing
// contracts, so the nominal row gives Nominal's doubles bit for bit (IEEE division and multiplication round as the
// compiler's constant folding does) — on the device and on the host alike.
__host__ __device__ inline Coeffs derive(const double *row) {
#pragma clang fp contract(off)
    const double m_mass = row[0], d1 = row[3], d2 = row[4], cd = row[11], rho = row[12], d = row[13], mu = row[16];
    const double w0 = row[18], b0 = row[20], t_def = row[21], t1 = row[22], m1 = row[24];
    Coeffs c;
    c.h0 = row[19];
    c.a = 0.14 + 0.36 * (b0 / w0) - 0.054 * (b0 / w0) * (b0 / w0);
    c.w0 = w0;
    c.b0 = b0;
    c.k = row[17];
    c.two_mu = 2.0 * mu;
    c.m0 = row[23];
    c.m1t = m1 * t_def;
    c.m2 = row[25];
    c.m3 = row[26];
    c.m4 = row[27];
    c.ps = row[14];
    c.pt = row[15];
    c.flow_c = kPi * d * cd;
    c.two_over_rho = 2.0 / rho;
    c.half_v1 = row[7] / 2;
    c.half_v2 = row[8] / 2;
    c.a1 = kPi * d1 * d1 / 4;
    c.a2 = kPi * d2 * d2 / 4;
    c.ft = row[2];
    c.press1 = 3 * kPi * d1 * d1 / 4;
    c.press2 = kPi * d2 * d2 / 2;
    c.b_damp = row[1];
    c.inv_m = 1.0 / m_mass;
    c.g = row[5];
    c.kb = row[6];
    c.kl_1 = row[9];
    c.kl_2 = row[10];
    c.inv_t1 = 1.0 / t1;
    return c;
}

template <class P>
constexpr bool kLiteral = false;   // P's members are literals: the expressions are left to the compiler as they always were
template <>
inline constexpr bool kLiteral<Nominal> = true;   // inline: the header is included by more than one translation unit

// M1 T + M2 log e + M3 log e_dot + M4 / e with its roundings spelled out — fma(M2, log e, M1 T), then the ROUNDED product
// M3 log e_dot added, then the quotient — which is what the compiler makes of the plain expression when the
// coefficients are literals (read off the nominal kernels' code). Left to contraction, coefficients in registers fuse the
// second product too; spelled out for Nominal as well, every existing kernel comes out with another schedule. So this
// one expression has two branches in forging_rhs: left to the compiler for literals, through here for run-time ones.
// Pinned by tests/test_gpu_press_params.py (test_nominal_plant_is_the_plant, test_nominal_bank_is_the_bank,
// test_nominal_projection_is_the_projection: bit-equality under the nominal row). If a compiler contracts the literal
// expression differently, those tests fail with differences of an ulp or so; to re-derive this function, dump the device
// assembly (scripts/isa_dump.sh), count v_fma_f64 / v_mul_f64 / v_add_f64 of plant_rk4_kernel<false> against
// plant_rk4_press_kernel<false> (equal apart from derive()'s own once the roundings agree), and read the order of the
// operations that feed the exponent's v_rndne_f64 in the nominal kernel.
__device__ __forceinline__ double flow_exponent(double m1t, double m2, double m3, double m4, double le, double led,
                                                double e) {
#pragma clang fp contract(off)
    const double t = m3 * led;
    return fma(m2, le, m1t) + t + m4 / e;
}

// FT * y_dot / 0.5 below the friction knee, never contracted: the quotient is 2 * round(FT * y_dot), which the compiler
// gives with a literal FT; with FT in a register it would otherwise fuse the doubling into fma(FT, y_dot, FT * y_dot),
// one rounding less, and the nominal row would no longer reproduce the nominal kernels.
__device__ __forceinline__ double knee_friction(double ft, double yd) {
#pragma clang fp contract(off)
    return ft * yd / 0.5;
}

// xdot = f(x, u), Functions.py:1633-1738 (SMOOTH: template_model.py:116-139); p: the press (above)
template <bool SMOOTH, class P = Nominal>
__device__ __forceinline__ void forging_rhs(const double (&x)[5], double u, double (&f)[5], P p = {}) {
    const double y = x[0], yd = x[1], z = x[4];
    double p1 = x[2], p2 = x[3];
    if (SMOOTH) {
        p1 = 0.5 * (p1 + sqrt(p1 * p1 + kSmoothEps));
        p2 = 0.5 * (p2 + sqrt(p2 * p2 + kSmoothEps));
    }
    // Fd_article = if_else(y > 0 && y_dot >= 0, Kd·Ad·M0·exp(M1 T)·e^M2·ė^M3·exp(M4/e), 0)   :1698-1704
    double fd = 0.0;
    if (y > 0.0 && yd >= 0.0) {
        const double rh = 1.0 / (p.h0 - y);                    // 1/h1
        const double r = p.h0 * rh;                            // H0/h1
        const double e = log(r);                             // strain, :1698
        const double ra = exp(p.a * e);                        // (H0/h1)^A
        const double w1 = p.w0 * ra;                           // :1673
        const double b1 = p.b0 * (1.0 + 0.67 * (r / ra - 1.0));   // :1674
        // Kd = K (1 + MU b1/(2y) + y/(4 b1)) over one division, :1686
        const double kd = p.k * (1.0 + (p.two_mu * b1 * b1 + y * y) / (4.0 * y * b1));
        const double ad = w1 * b1;                           // :1687
        const double ed = yd * rh;                           // e_dot, :1699
        if constexpr (kLiteral<P>)
            fd = kd * ad * p.m0 * exp(p.m1t + p.m2 * log(e) + p.m3 * log(ed) + p.m4 / e);
        else
            fd = kd * ad * p.m0 * exp(flow_exponent(p.m1t, p.m2, p.m3, p.m4, log(e), log(ed), e));
    }
    // servo-valve flows, :1709-1719: the spool direction picks the pressure differences
    const bool work = z >= 0.0;
    const double apb = work ? p.ps - p1 : p1 - p.pt;
    const double aat = work ? p2 - p.pt : p.ps - p2;
    const double qpb = p.flow_c * z * copysign(sqrt(p.two_over_rho * fabs(apb)), apb);
    const double qat = p.flow_c * z * copysign(sqrt(p.two_over_rho * fabs(aat)), aat);
    const double v1 = p.half_v1 + p.a1 * y;                     // :1722-1723
    const double v2 = p.half_v2 - p.a2 * y;
    const double ft = fabs(yd) <= 0.5 ? knee_friction(p.ft, yd) : p.ft;  // :1726
    f[0] = yd;                                               // :1729-1733
    f[1] = (p.press1 * p1 - p.press2 * p2 - p.b_damp * yd - ft - fd) * p.inv_m + p.g;
    f[2] = p.kb / v1 * (qpb * (1.0 / 3.0) - p.a1 * yd - p.kl_1 * p1);
    f[3] = p.kb / v2 * (-0.5 * qat + p.a2 * yd - p.kl_2 * p2);
    f[4] = (u - z) * p.inv_t1;
}

// One TS step of Ruge_Kuta (Functions.py:1758-1776): `substeps` RK4 stages of dt = TS/substeps.
// NOISE: the step under process noise w[5] in the units of xdot: do-mpc adds the w of a `process_noise=True` state to
// its right-hand side (template_model.py:145-149) and the harness holds one draw over the whole sampling step
// (Functions.py:1176-1183), so EVERY stage of every sub-step evaluates k = f(x, u) + w (not x + TS·w after the step).
// w is constant over the step, so its share of each stage state and of the update is a term of its own —
// x + c (f + w) = (x + c f) + c w, and dt/6 (6 w) = dt w — added AFTER the expressions of the noise-free step: with
// w = 0 every one of them, however the compiler contracts it, is followed by + 0, and the step is the noise-free one
// bit for bit (plus_noise: that trailing term). Without NOISE w is not read.
template <bool NOISE>
__device__ __forceinline__ double plus_noise(double a, double cw) { return NOISE ? a + cw : a; }

template <bool SMOOTH, bool NOISE = false, class P = Nominal>
__device__ __forceinline__ void rk4_step(double (&x)[5], double u, double dt, int substeps, const double *w = nullptr,
                                         P p = {}) {
    double hw[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, dw[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (NOISE) {
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            hw[i] = dt / 2 * w[i];
            dw[i] = dt * w[i];
        }
    }
    for (int m = 0; m < substeps; ++m) {
        double k1[5], k2[5], k3[5], k4[5], xs[5];
        forging_rhs<SMOOTH>(x, u, k1, p);
#pragma unroll
        for (int i = 0; i < 5; ++i) xs[i] = plus_noise<NOISE>(x[i] + dt / 2 * k1[i], hw[i]);
        forging_rhs<SMOOTH>(xs, u, k2, p);
#pragma unroll
        for (int i = 0; i < 5; ++i) xs[i] = plus_noise<NOISE>(x[i] + dt / 2 * k2[i], hw[i]);
        forging_rhs<SMOOTH>(xs, u, k3, p);
#pragma unroll
        for (int i = 0; i < 5; ++i) xs[i] = plus_noise<NOISE>(x[i] + dt * k3[i], dw[i]);
        forging_rhs<SMOOTH>(xs, u, k4, p);
#pragma unroll
        for (int i = 0; i < 5; ++i) x[i] = plus_noise<NOISE>(x[i] + dt / 6 * (k1[i] + 2 * k2[i] + 2 * k3[i] + k4[i]), dw[i]);
    }
}

constexpr int kPlantBlock = 256;

// x (B, S+1, 5): x[b, 0] = x0[b], x[b, t+1] = F(x[b, t], u[b, t]) for u (B, S)
template <bool SMOOTH>
__global__ __launch_bounds__(kPlantBlock) void plant_rk4_kernel(int B, int S, double dt, int substeps,
                                                                const double *__restrict__ x0,
                                                                const double *__restrict__ u,
                                                                double *__restrict__ xo) {
    const int b = blockIdx.x * kPlantBlock + threadIdx.x;
    if (b >= B) return;
    double x[5];
    double *o = xo + (size_t)b * (S + 1) * 5;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        x[i] = x0[(size_t)b * 5 + i];
        o[i] = x[i];
    }
    const double *ub = u + (size_t)b * S;
    double un = S > 0 ? ub[0] : 0.0;
    for (int t = 0; t < S; ++t) {
        const double ut = un;
        if (t + 1 < S) un = ub[t + 1];                       // next command in flight during the step
        rk4_step<SMOOTH>(x, ut, dt, substeps);
        o += 5;
#pragma unroll
        for (int i = 0; i < 5; ++i) o[i] = x[i];
    }
}

// (The body is repeated, not shared: called from one __device__ function taking the policy, plant_rk4_kernel comes out
// with two moves rescheduled and another register for the row pointer — the same work, but no longer the parent's
// instructions, which DESIGN.md §7.11 promises. The same holds for the two projection kernels in fcr_feasibility.h.)
// plant_rk4_kernel with every trajectory's own press: lane b derives its coefficients from row b * stride_traj of
// `press` (kPressFields doubles per row; stride 0: one row shared by every trajectory) and keeps them in registers.
template <bool SMOOTH>
__global__ __launch_bounds__(kPlantBlock) void plant_rk4_press_kernel(int B, int S, double dt, int substeps,
                                                                      const double *__restrict__ x0,
                                                                      const double *__restrict__ u,
                                                                      double *__restrict__ xo,
                                                                      const double *__restrict__ press,
                                                                      long long stride_traj) {
    const int b = blockIdx.x * kPlantBlock + threadIdx.x;
    if (b >= B) return;
    const LaneParams p = derive(press + (size_t)b * stride_traj);
    double x[5];
    double *o = xo + (size_t)b * (S + 1) * 5;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        x[i] = x0[(size_t)b * 5 + i];
        o[i] = x[i];
    }
    const double *ub = u + (size_t)b * S;
    double un = S > 0 ? ub[0] : 0.0;
    for (int t = 0; t < S; ++t) {
        const double ut = un;
        if (t + 1 < S) un = ub[t + 1];                       // next command in flight during the step
        rk4_step<SMOOTH, false>(x, ut, dt, substeps, nullptr, p);
        o += 5;
#pragma unroll
        for (int i = 0; i < 5; ++i) o[i] = x[i];
    }
}

}  // namespace plant
}  // namespace fcr
