// Scalar oracle of the Sim3 pose graph (rumi_essential_graph, rumi_sim3_correct_points; include/rumi_opt.h): g2o's Levenberg-Marquardt with
// setUserLambdaInit(1e-16) over VertexSim3Expmap / EdgeSim3 with numeric Jacobians, dense LL^T in vertex order, in its own scalar code.
// It restates the same upstream formulas as the product (G/types/sim3.h: the coefficients of exp and log and their branches), so a shared
// misreading of those would not show in a device-against-oracle comparison: tests/test_essential_cpu.py checks the general branch against
// the matrix logarithm; the small-angle branches rest on the reading of sim3.h alone.  Built by tests/essential_scene.py.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

namespace {
struct Q { double x, y, z, w; };
struct V3 { double x, y, z; };
struct Sim { Q r; V3 t; double s; };

Q qmul(Q a, Q b) {
    return {a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z,
            a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
V3 qrot(Q q, V3 v) {                                         // v + 2 w (u x v) + 2 u x (u x v)
    const V3 u{q.x, q.y, q.z};
    V3 uv = cross(u, v);
    uv = {uv.x + uv.x, uv.y + uv.y, uv.z + uv.z};
    const V3 c = cross(u, uv);
    return {v.x + q.w * uv.x + c.x, v.y + q.w * uv.y + c.y, v.z + q.w * uv.z + c.z};
}
void qmat(Q q, double R[3][3]) {
    const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z, twx = tx * q.w, twy = ty * q.w, twz = tz * q.w, txx = tx * q.x, txy = ty * q.x,
                 txz = tz * q.x, tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    R[0][0] = 1 - (tyy + tzz); R[0][1] = txy - twz; R[0][2] = txz + twy;
    R[1][0] = txy + twz; R[1][1] = 1 - (txx + tzz); R[1][2] = tyz - twx;
    R[2][0] = txz - twy; R[2][1] = tyz + twx; R[2][2] = 1 - (txx + tyy);
}
Q matq(const double R[3][3]) {                               // Eigen's Quaternion(Matrix3)
    Q q;
    double t = R[0][0] + R[1][1] + R[2][2];
    if (t > 0) {
        t = std::sqrt(t + 1.0);
        q.w = 0.5 * t; t = 0.5 / t;
        q.x = (R[2][1] - R[1][2]) * t; q.y = (R[0][2] - R[2][0]) * t; q.z = (R[1][0] - R[0][1]) * t;
        return q;
    }
    int i = 0;
    if (R[1][1] > R[0][0]) i = 1;
    if (R[2][2] > R[i][i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(R[i][i] - R[j][j] - R[k][k] + 1.0);
    double v[3];
    v[i] = 0.5 * t; t = 0.5 / t;
    q.w = (R[k][j] - R[j][k]) * t;
    v[j] = (R[j][i] + R[i][j]) * t; v[k] = (R[k][i] + R[i][k]) * t;
    q.x = v[0]; q.y = v[1]; q.z = v[2];
    return q;
}
Sim from8(const double *S) { return {{S[0], S[1], S[2], S[3]}, {S[4], S[5], S[6]}, S[7]}; }
void to8(const Sim &S, double *o) { o[0] = S.r.x; o[1] = S.r.y; o[2] = S.r.z; o[3] = S.r.w; o[4] = S.t.x; o[5] = S.t.y; o[6] = S.t.z; o[7] = S.s; }
V3 smap(const Sim &S, V3 p) { const V3 r = qrot(S.r, p); return {S.s * r.x + S.t.x, S.s * r.y + S.t.y, S.s * r.z + S.t.z}; }
Sim smul(const Sim &a, const Sim &b) { const V3 r = qrot(a.r, b.t); return {qmul(a.r, b.r), {a.s * r.x + a.t.x, a.s * r.y + a.t.y, a.s * r.z + a.t.z}, a.s * b.s}; }
Sim sinv(const Sim &a) {
    const Q c{-a.r.x, -a.r.y, -a.r.z, a.r.w};
    const double k = -1. / a.s;
    return {c, qrot(c, {k * a.t.x, k * a.t.y, k * a.t.z}), 1. / a.s};
}
// the coefficients shared by exp and log: W = A Omega + B Omega^2 + C I
void abc(double sigma, double s, double theta, bool smallT, double &A, double &B, double &C) {
    const double eps = 0.00001;
    if (std::fabs(sigma) < eps) {
        C = 1;
        if (smallT) { A = 0.5; B = 1. / 6.; }
        else { const double t2 = theta * theta; A = (1 - std::cos(theta)) / t2; B = (theta - std::sin(theta)) / (t2 * theta); }
    } else {
        C = (s - 1) / sigma;
        if (smallT) { const double g2 = sigma * sigma; A = ((sigma - 1) * s + 1) / g2; B = ((0.5 * g2 - sigma + 1) * s) / (g2 * sigma); }
        else {
            const double a = s * std::sin(theta), b = s * std::cos(theta), t2 = theta * theta, c = t2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / t2;
        }
    }
}
void skew2(const double w[3], double O[3][3], double O2[3][3]) {
    const double o[3][3] = {{0, -w[2], w[1]}, {w[2], 0, -w[0]}, {-w[1], w[0], 0}};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) { O[i][j] = o[i][j]; O2[i][j] = o[i][0] * o[0][j] + o[i][1] * o[1][j] + o[i][2] * o[2][j]; }
}
Sim sexp(const double u[7]) {
    const double theta = std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]), sigma = u[6], s = std::exp(sigma);
    const bool smallT = theta < 0.00001;
    double O[3][3], O2[3][3], A, B, C, R[3][3], W[3][3];
    skew2(u, O, O2);
    abc(sigma, s, theta, smallT, A, B, C);
    const double ra = smallT ? 1.0 : std::sin(theta) / theta, rb = smallT ? 1.0 : (1 - std::cos(theta)) / (theta * theta);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const double I = i == j;
            R[i][j] = smallT ? (I + O[i][j]) + O2[i][j] : (I + ra * O[i][j]) + rb * O2[i][j];
            W[i][j] = (A * O[i][j] + B * O2[i][j]) + C * I;
        }
    Sim S;
    S.r = matq(R);
    S.t = {W[0][0] * u[3] + W[0][1] * u[4] + W[0][2] * u[5], W[1][0] * u[3] + W[1][1] * u[4] + W[1][2] * u[5], W[2][0] * u[3] + W[2][1] * u[4] + W[2][2] * u[5]};
    S.s = s;
    return S;
}
void slog(const Sim &S, double out[7]) {
    const double sigma = std::log(S.s);
    double R[3][3];
    qmat(S.r, R);
    const double d = 0.5 * (R[0][0] + R[1][1] + R[2][2] - 1);
    const bool smallT = d > 1 - 0.00001;
    double theta = 0, k = 0.5;
    if (!smallT) { theta = std::acos(d); k = theta / (2 * std::sqrt(1 - d * d)); }
    const double w[3] = {k * (R[2][1] - R[1][2]), k * (R[0][2] - R[2][0]), k * (R[1][0] - R[0][1])};
    double O[3][3], O2[3][3], A, B, C, M[3][4];
    skew2(w, O, O2);
    abc(sigma, S.s, theta, smallT, A, B, C);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) M[i][j] = (A * O[i][j] + B * O2[i][j]) + (i == j ? C : 0.0);
    M[0][3] = S.t.x; M[1][3] = S.t.y; M[2][3] = S.t.z;
    for (int c = 0; c < 3; c++) {                            // W upsilon = t by elimination with row pivoting
        int p = c;
        for (int r = c + 1; r < 3; r++) if (std::fabs(M[r][c]) > std::fabs(M[p][c])) p = r;
        if (p != c) for (int j = 0; j < 4; j++) std::swap(M[c][j], M[p][j]);
        for (int r = c + 1; r < 3; r++) { const double f = M[r][c] / M[c][c]; for (int j = c + 1; j < 4; j++) M[r][j] -= f * M[c][j]; }
    }
    double u[3];
    for (int r = 2; r >= 0; r--) { double t = M[r][3]; for (int j = r + 1; j < 3; j++) t -= M[r][j] * u[j]; u[r] = t / M[r][r]; }
    out[0] = w[0]; out[1] = w[1]; out[2] = w[2]; out[3] = u[0]; out[4] = u[1]; out[5] = u[2]; out[6] = sigma;
}
void edge_error(const Sim &C, const Sim &S0, const Sim &S1, double e[7]) { slog(smul(smul(C, S0), sinv(S1)), e); }
Sim oplus(const Sim &S, const double *dx, bool fixScale) {
    double u[7];
    for (int i = 0; i < 7; i++) u[i] = dx[i];
    if (fixScale) u[6] = 0;
    return smul(sexp(u), S);
}

struct Graph {
    int nV, nE, nR, n;
    std::vector<Sim> S, C;
    std::vector<int> v0, v1, col;
    const uint8_t *fixed, *fixScale;
};
// active sets: an edge with two fixed ends is dropped, a free vertex with an edge owns rows (vertex order)
Graph make_graph(int nV, const double *S8, const uint8_t *fixed, const uint8_t *fixScale, int nE, const int32_t *v0, const int32_t *v1, const double *meas) {
    Graph G;
    G.nV = nV; G.fixed = fixed; G.fixScale = fixScale;
    for (int v = 0; v < nV; v++) G.S.push_back(from8(S8 + 8 * v));
    std::vector<int> deg(nV, 0);
    for (int e = 0; e < nE; e++) {
        if (fixed[v0[e]] && fixed[v1[e]]) continue;
        G.v0.push_back(v0[e]); G.v1.push_back(v1[e]); G.C.push_back(from8(meas + 8 * e));
        deg[v0[e]]++; deg[v1[e]]++;
    }
    G.nE = (int)G.v0.size();
    G.col.assign(nV, -1);
    G.nR = 0;
    for (int v = 0; v < nV; v++) if (!fixed[v] && deg[v] > 0) G.col[v] = G.nR++;
    G.n = 7 * G.nR;
    return G;
}
double chi2(const Graph &G, const std::vector<Sim> &S) {
    double c = 0;
    for (int e = 0; e < G.nE; e++) {
        double r[7];
        edge_error(G.C[e], S[G.v0[e]], S[G.v1[e]], r);
        double a = 0;
        for (int i = 0; i < 7; i++) a += r[i] * r[i];
        c += a;
    }
    return c;
}
// H (dense, n x n, both triangles) and b = -J^T e, Jacobians by central differences of 1e-9 through oplus
void build(const Graph &G, const std::vector<Sim> &S, std::vector<double> &H, std::vector<double> &b) {
    const int n = G.n;
    H.assign((size_t)n * n, 0.0); b.assign(n, 0.0);
    const double delta = 1e-9, scalar = 1.0 / (2 * delta);
    for (int e = 0; e < G.nE; e++) {
        const int vs[2] = {G.v0[e], G.v1[e]};
        double J[2][7][7] = {}, r[7];
        edge_error(G.C[e], S[vs[0]], S[vs[1]], r);
        for (int end = 0; end < 2; end++) {
            const int v = vs[end];
            if (G.fixed[v]) continue;
            for (int d = 0; d < 7; d++) {
                double u[7] = {0, 0, 0, 0, 0, 0, 0}, ep[7], em[7];
                u[d] = delta;
                const Sim Sp = oplus(S[v], u, G.fixScale[v]);
                edge_error(G.C[e], end ? S[vs[0]] : Sp, end ? Sp : S[vs[1]], ep);
                u[d] = -delta;
                const Sim Sm = oplus(S[v], u, G.fixScale[v]);
                edge_error(G.C[e], end ? S[vs[0]] : Sm, end ? Sm : S[vs[1]], em);
                for (int i = 0; i < 7; i++) J[end][i][d] = scalar * (ep[i] - em[i]);
            }
        }
        for (int a = 0; a < 2; a++) {
            const int ra = G.col[vs[a]];
            if (ra < 0) continue;
            for (int i = 0; i < 7; i++) {
                double t = 0;
                for (int k = 0; k < 7; k++) t += J[a][k][i] * r[k];
                b[7 * ra + i] += -t;
            }
            for (int c = 0; c < 2; c++) {
                const int rc = G.col[vs[c]];
                if (rc < 0) continue;
                for (int i = 0; i < 7; i++)
                    for (int j = 0; j < 7; j++) {
                        double t = 0;
                        for (int k = 0; k < 7; k++) t += J[a][k][i] * J[c][k][j];
                        H[(size_t)(7 * ra + i) * n + 7 * rc + j] += t;
                    }
            }
        }
    }
}
// (H + lambda I) x = b by dense LL^T; false when a pivot is not positive and finite
bool solve(const std::vector<double> &H, const std::vector<double> &b, double lambda, int n, std::vector<double> &x) {
    std::vector<double> L((size_t)n * n, 0.0), y(n);
    for (int j = 0; j < n; j++) {
        double d = H[(size_t)j * n + j] + lambda;
        for (int k = 0; k < j; k++) d -= L[(size_t)j * n + k] * L[(size_t)j * n + k];
        if (!(d > 0) || !std::isfinite(d)) return false;
        const double l = std::sqrt(d);
        L[(size_t)j * n + j] = l;
        for (int i = j + 1; i < n; i++) {
            double t = H[(size_t)i * n + j];
            for (int k = 0; k < j; k++) t -= L[(size_t)i * n + k] * L[(size_t)j * n + k];
            L[(size_t)i * n + j] = t / l;
        }
    }
    for (int i = 0; i < n; i++) { double t = b[i]; for (int k = 0; k < i; k++) t -= L[(size_t)i * n + k] * y[k]; y[i] = t / L[(size_t)i * n + i]; }
    x.assign(n, 0.0);
    for (int i = n - 1; i >= 0; i--) { double t = y[i]; for (int k = i + 1; k < n; k++) t -= L[(size_t)k * n + i] * x[k]; x[i] = t / L[(size_t)i * n + i]; }
    return true;
}
}  // namespace

extern "C" {
void ego_error(const double *C8, const double *S0, const double *S1, double *e7) { edge_error(from8(C8), from8(S0), from8(S1), e7); }
void ego_exp(const double *u7, double *S8) { to8(sexp(u7), S8); }
void ego_log(const double *S8, double *u7) { slog(from8(S8), u7); }
void ego_mul(const double *A8, const double *B8, double *o8) { to8(smul(from8(A8), from8(B8)), o8); }
void ego_inverse(const double *A8, double *o8) { to8(sinv(from8(A8)), o8); }

// H [n x n], b [n], col [nV] of the current state, and the solution of (H + lambda I) x = b; returns n (or -1 when the factorisation fails)
int ego_linear_system(int nV, const double *S8, const uint8_t *fixed, const uint8_t *fixScale, int nE, const int32_t *v0, const int32_t *v1,
                      const double *meas, double lambda, double *H_out, double *b_out, int32_t *col_out, double *x_out) {
    const Graph G = make_graph(nV, S8, fixed, fixScale, nE, v0, v1, meas);
    std::vector<double> H, b, x;
    build(G, G.S, H, b);
    const bool ok = solve(H, b, lambda, G.n, x);
    std::memcpy(H_out, H.data(), H.size() * 8); std::memcpy(b_out, b.data(), b.size() * 8);
    for (int v = 0; v < nV; v++) col_out[v] = G.col[v];
    if (ok) std::memcpy(x_out, x.data(), x.size() * 8);
    return ok ? G.n : -1;
}

// rumi_essential_graph; besides its outputs: the smallest |rho| over all trials and, per iteration, (iniChi - currentChi) * 1e3 / iniChi
int ego_essential_graph(int nV, double *S_io8, const uint8_t *fixed, const uint8_t *fixScale, int nE, const int32_t *v0, const int32_t *v1,
                        const double *meas, int nIter, int32_t *stats, double *trace, double *min_abs_rho, double *ratios) {
    const double kNaN = std::numeric_limits<double>::quiet_NaN();
    for (int i = 0; i <= nIter; i++) trace[i] = kNaN;
    for (int i = 0; i < nIter; i++) ratios[i] = kNaN;
    for (int i = 0; i < 4; i++) stats[i] = 0;
    *min_abs_rho = std::numeric_limits<double>::infinity();
    Graph G = make_graph(nV, S_io8, fixed, fixScale, nE, v0, v1, meas);
    if (G.nE == 0) return 0;
    const int n = G.n;
    double lambda = 1e-16, ni = 2, currentChi = 0;
    int nBad = 0, iters = 0, trials = 0, how = 0;
    std::vector<double> H, b, x;
    for (int it = 0; it < nIter; it++) {
        if (it == 0) { currentChi = chi2(G, G.S); trace[0] = currentChi; }
        const double iniChi = currentChi;
        build(G, G.S, H, b);
        double rho = 0;
        int qmax = 0;
        do {
            const bool ok = solve(H, b, lambda, n, x);
            if (!ok) x.assign(n, 0.0);
            std::vector<Sim> T = G.S;
            for (int v = 0; v < nV; v++) if (G.col[v] >= 0) T[v] = oplus(G.S[v], &x[7 * G.col[v]], G.fixScale[v]);
            double tempChi = chi2(G, T);
            if (!ok) tempChi = DBL_MAX;
            double scale = 0;
            for (int j = 0; j < n; j++) scale += x[j] * (lambda * x[j] + b[j]);
            rho = (currentChi - tempChi) / (scale + 1e-3);
            if (std::fabs(rho) < *min_abs_rho) *min_abs_rho = std::fabs(rho);
            if (rho > 0 && std::isfinite(tempChi)) {
                double alpha = 1. - std::pow(2 * rho - 1, 3);
                if (alpha > 2. / 3.) alpha = 2. / 3.;
                lambda *= alpha < 1. / 3. ? 1. / 3. : alpha;
                ni = 2;
                currentChi = tempChi;
                G.S = T;
            } else { lambda *= ni; ni *= 2; }
            qmax++; trials++;
        } while (rho < 0 && qmax < 10);
        iters++;
        trace[iters] = currentChi;
        ratios[it] = (iniChi - currentChi) * 1e3 / iniChi;
        if (qmax == 10 || rho == 0) { how = 1; break; }
        if ((iniChi - currentChi) * 1e3 < iniChi) nBad++; else nBad = 0;
        if (nBad >= 3) { how = 2; break; }
    }
    for (int v = 0; v < nV; v++) if (G.col[v] >= 0) to8(G.S[v], S_io8 + 8 * v);
    stats[0] = iters; stats[1] = trials; stats[2] = G.nR; stats[3] = how;
    return 0;
}

// rumi_sim3_correct_points
void ego_correct_points(int mode, int n, float *X, const int32_t *ref, const void *tabA, const void *tabB) {
    for (int i = 0; i < n; i++) {
        const int v = ref[i];
        if (v < 0) continue;
        float *x = X + 3 * i;
        if (mode == 0) {
            const V3 p = smap(from8((const double *)tabB + 8 * v), smap(from8((const double *)tabA + 8 * v), {(double)x[0], (double)x[1], (double)x[2]}));
            x[0] = (float)p.x; x[1] = (float)p.y; x[2] = (float)p.z;
        } else {                                             // 4 x 4 float matrices: M = Twr * TNonCorrectedwr^-1, then M * X
            const float *ta = (const float *)tabA + 7 * v, *tb = (const float *)tabB + 7 * v;
            double Rd[3][3];
            float Ra[3][3], Rb[3][3], M[3][3], t[3];
            qmat({ta[0], ta[1], ta[2], ta[3]}, Rd);
            for (int a = 0; a < 3; a++) for (int c = 0; c < 3; c++) Ra[a][c] = (float)Rd[a][c];
            qmat({tb[0], tb[1], tb[2], tb[3]}, Rd);
            for (int a = 0; a < 3; a++) for (int c = 0; c < 3; c++) Rb[a][c] = (float)Rd[a][c];
            for (int a = 0; a < 3; a++) {
                for (int c = 0; c < 3; c++) M[a][c] = Ra[a][0] * Rb[c][0] + Ra[a][1] * Rb[c][1] + Ra[a][2] * Rb[c][2];     // Ra Rb^T
                t[a] = ta[4 + a] - (M[a][0] * tb[4] + M[a][1] * tb[5] + M[a][2] * tb[6]);
            }
            const float p[3] = {x[0], x[1], x[2]};
            for (int a = 0; a < 3; a++) x[a] = M[a][0] * p[0] + M[a][1] * p[1] + M[a][2] * p[2] + t[a];
        }
    }
}
}
