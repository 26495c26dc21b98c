// batched dense factorisation for the Laplace posterior: k_chol_factor, k_tri_inverse
// Part of pglm_kernels.hip.h (included from there, in order; one translation unit).
#pragma once
// ---------------------------------------------------------------------------
// A = minus the Hessian of the log posterior of every neuron, (M, P, ld) f64 on the device (k_hess leaves both triangles;
// only the lower one is read here).  k_chol_factor equilibrates and factors in place, C = D^-1/2 A D^-1/2 = Ls Ls^T with
// D = diag A (laplace_from_hessian's scaling: at a group-lasso optimum curvatures sit many orders of magnitude apart),
// k_tri_inverse overwrites Ls with Ls^-1.  One workgroup of 256 threads per matrix, everything in tiles of 32 columns:
// at P = 641 a matrix is 3.3 MB and lives in L2 while its workgroup walks it, at P = 1221 it is 12 MB; no full-height
// panel is ever held in LDS.  All f64, plain FMA (88 MFLOP per matrix at P = 641 against 128 independent matrices: the
// matrix cores would buy nothing that matters), no atomics, every sum in an order that depends on P alone, and a
// workgroup touches its own matrix only: batch = subset, repeat = same bits.
//
// factor, right-looking, for every block column k0 (32 wide):
//   1. the diagonal block is factored in LDS (one column at a time, three barriers each);
//   2. every row below it is solved against that block by ONE thread (x D^T = c, forward substitution, 128 rows in LDS);
//   3. the trailing lower triangle is updated in 64 x 64 tiles, C[I, J] -= Lp[I] Lp[J]^T, 4 x 4 outputs per thread, the
//      two 64 x 32 panel tiles staged in LDS.
// A diagonal entry or a pivot that is non-finite or <= 0 raises a flag in LDS (the first such column + 1) and every loop
// runs on to its uniform end on whatever numbers there are: no thread leaves a loop that holds a barrier.
//
// inverse, Higham's Method 1B (Accuracy and Stability, ch. 14.3: the blocked method with the RIGHT residual bound
// |Ls X - I| <= c u |Ls| |X|, what a substitution gives): for block columns J left to right and row tiles I >= J top down
//     X[I, J] = Ls[I, I]^-1 (delta_IJ - sum_{J <= K < I} Ls[I, K] X[K, J])
// the sum as 32 x 32 tile products by all threads, the solve with the diagonal block by forward substitution, one thread
// per column.  In place: tile (I, J) is overwritten after its last use as Ls, and the columns right of J are untouched.
// ---------------------------------------------------------------------------

#define PGL_CH_NB 32                           // block column width; the diagonal block in LDS
#define PGL_CH_TILE 64                         // rows / columns of a trailing tile of the factor
#define PGL_CH_PAD 33                          // LDS row stride in doubles (bank-conflict-free column walks)

__global__ __launch_bounds__(256) void k_chol_factor(double* __restrict__ A, const int P, const int ld,
                                                     double* __restrict__ scale, double* __restrict__ logdet,
                                                     int* __restrict__ info)
{
    __shared__ double D[PGL_CH_NB][PGL_CH_PAD];
    __shared__ double T[2 * PGL_CH_TILE][PGL_CH_PAD];           // the panel solve's rows; the update's two panel tiles
    double (*As)[PGL_CH_PAD] = T, (*Bs)[PGL_CH_PAD] = T + PGL_CH_TILE;
    __shared__ double red[4];
    __shared__ int flag;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ty = tid >> 4, tx = tid & 15;
    double* Am = A + (size_t)blockIdx.x * P * ld;
    double* sc = scale + (size_t)blockIdx.x * P;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);

    // the diagonal: scales, sum log A_ii, the first entry that cannot be scaled (its scale is 1: the pivot fails there)
    double la = 0.0, bad = 1e300;
    for (int i = tid; i < P; i += 256) {
        const double a = Am[(size_t)i * ld + i];
        const bool ok = a > 0.0 && a < __builtin_huge_val();
        if (!ok && bad > (double)i) bad = (double)i;
        sc[i] = ok ? sqrt(a) : 1.0;
        la += ok ? log(a) : 0.0;
    }
    bad = -pgl_blk_max(-bad, red);
    if (tid == 0) flag = bad < 1e299 ? (int)bad + 1 : 0;
    __syncthreads();
    // C = D^-1/2 A D^-1/2 over the lower triangle, in place: (a_ij r_i) r_j, r = 1 / sqrt(a_ii).  The reciprocals are taken
    // once into LDS (T is free until the first panel) where P of them fit, else per element: the same numbers either way
    double* rinv = &T[0][0];
    const bool staged = P <= 2 * PGL_CH_TILE * PGL_CH_PAD;
    if (staged) {
        for (int i = tid; i < P; i += 256) rinv[i] = 1.0 / sc[i];
        __syncthreads();
    }
    for (int i = wave; i < P; i += 4) {
        const double ri = staged ? rinv[i] : 1.0 / sc[i];
        double* row = Am + (size_t)i * ld;
        for (int j = lane; j <= i; j += 64) row[j] = (row[j] * ri) * (staged ? rinv[j] : 1.0 / sc[j]);
    }
    __syncthreads();

    for (int k0 = 0; k0 < P; k0 += PGL_CH_NB) {
        const int nb = min(PGL_CH_NB, P - k0);
        // 1. the diagonal block
        for (int e = tid; e < PGL_CH_NB * PGL_CH_NB; e += 256) {
            const int i = e >> 5, c = e & 31;
            D[i][c] = (i < nb && c <= i) ? Am[(size_t)(k0 + i) * ld + k0 + c] : 0.0;
        }
        __syncthreads();
        for (int j = 0; j < nb; ++j) {
            if (tid == 0) {
                const double p = D[j][j];
                if (!(p > 0.0 && p < __builtin_huge_val()) && (flag == 0 || k0 + j + 1 < flag)) flag = k0 + j + 1;
                D[j][j] = sqrt(p);
            }
            __syncthreads();
            if (tid > j && tid < nb) D[tid][j] /= D[j][j];
            __syncthreads();
            for (int e = tid; e < PGL_CH_NB * PGL_CH_NB; e += 256) {
                const int i = e >> 5, c = e & 31;
                if (c > j && c <= i && i < nb) D[i][c] = fma(-D[i][j], D[c][j], D[i][c]);
            }
            __syncthreads();
        }
        for (int e = tid; e < PGL_CH_NB * PGL_CH_NB; e += 256) {
            const int i = e >> 5, c = e & 31;
            if (i < nb && c <= i) Am[(size_t)(k0 + i) * ld + k0 + c] = D[i][c];
        }
        const int t0 = k0 + PGL_CH_NB;                           // first row below the block (then nb = 32)
        if (t0 >= P) break;                                      // (uniform)
        // 2. the panel, 128 rows at a time through LDS: thread r solves x D^T = c for row r in place (rolled loops on LDS:
        //    a register copy of the row unrolls into more live values than a thread has registers)
        for (int R0 = t0; R0 < P; R0 += 2 * PGL_CH_TILE) {
            for (int e = tid; e < 2 * PGL_CH_TILE * PGL_CH_NB; e += 256) {
                const int i = e >> 5, c = e & 31;
                T[i][c] = (R0 + i < P) ? Am[(size_t)(R0 + i) * ld + k0 + c] : 0.0;
            }
            __syncthreads();
            if (tid < 2 * PGL_CH_TILE) {
                double* x = T[tid];
                for (int j = 0; j < PGL_CH_NB; ++j) {
                    double s = x[j];
                    for (int l = 0; l < j; ++l) s = fma(-x[l], D[j][l], s);
                    x[j] = s / D[j][j];
                }
            }
            __syncthreads();
            for (int e = tid; e < 2 * PGL_CH_TILE * PGL_CH_NB; e += 256) {
                const int i = e >> 5, c = e & 31;
                if (R0 + i < P) Am[(size_t)(R0 + i) * ld + k0 + c] = T[i][c];
            }
            __syncthreads();
        }
        // 3. the trailing lower triangle, tile (I0, J0), I0 >= J0: element (i, j), j <= i, loses sum_k Lp[i][k] Lp[j][k]
        for (int J0 = t0; J0 < P; J0 += PGL_CH_TILE) {
            for (int e = tid; e < PGL_CH_TILE * PGL_CH_NB; e += 256) {
                const int i = e >> 5, c = e & 31;
                Bs[i][c] = (J0 + i < P) ? Am[(size_t)(J0 + i) * ld + k0 + c] : 0.0;
            }
            for (int I0 = J0; I0 < P; I0 += PGL_CH_TILE) {
                for (int e = tid; e < PGL_CH_TILE * PGL_CH_NB; e += 256) {
                    const int i = e >> 5, c = e & 31;
                    As[i][c] = (I0 + i < P) ? Am[(size_t)(I0 + i) * ld + k0 + c] : 0.0;
                }
                __syncthreads();
                double c[4][4];
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int i = I0 + ty + 16 * a, j = J0 + tx + 16 * b;
                        c[a][b] = (i < P && j <= i) ? Am[(size_t)i * ld + j] : 0.0;
                    }
#pragma unroll 4
                for (int k = 0; k < PGL_CH_NB; ++k) {
                    double av[4], bv[4];
#pragma unroll
                    for (int a = 0; a < 4; ++a) av[a] = As[ty + 16 * a][k];
#pragma unroll
                    for (int b = 0; b < 4; ++b) bv[b] = Bs[tx + 16 * b][k];
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b) c[a][b] = fma(-av[a], bv[b], c[a][b]);
                }
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const int i = I0 + ty + 16 * a, j = J0 + tx + 16 * b;
                        if (i < P && j <= i) Am[(size_t)i * ld + j] = c[a][b];
                    }
                __syncthreads();                                 // As (and, after the last I0, Bs) is free again
            }
        }
    }
    __syncthreads();
    // log det A = 2 sum log Ls_ii + sum log A_ii; a failed row is NaN throughout
    const int f = flag;
    double ls = la;
    for (int i = tid; i < P; i += 256) ls += 2.0 * log(Am[(size_t)i * ld + i]);
    ls = pgl_blk_sum(ls, red);
    if (f != 0) {
        for (int i = wave; i < P; i += 4) {
            double* row = Am + (size_t)i * ld;
            for (int j = lane; j <= i; j += 64) row[j] = nan;
        }
        for (int i = tid; i < P; i += 256) sc[i] = nan;
    }
    if (tid == 0) {
        logdet[blockIdx.x] = f != 0 ? nan : ls;
        info[blockIdx.x] = f;
    }
}

// solve against the factor, x = D^-1/2 Ls^-T Ls^-1 D^-1/2 b (the Newton direction of pglm_newton.hip.h: 2 P^2 flops where
// the inverse costs P^3 / 3 and two products).  One workgroup per matrix, blocks of 32 like the factor, the vector in the
// caller's x row throughout (b and x may be the same memory: every element is read by the thread that writes it).  Both
// substitutions are left-looking, so that every pass over Ls runs along its rows:
//   forward,  block K top down:   r_K = y_K - sum_{c < k0} Ls[K, c] y_c   one wave per row, lanes along the columns, a wave64
//             butterfly per row; then Ls[K, K] y_K = r_K in the first wave, the block's vector in registers (lane i holds
//             y_i, a shuffle hands the finished y_j down), the diagonal block in LDS;
//   backward, block K bottom up:  r_K = x_K - sum_{i >= k0 + 32} Ls[i, K]^T x_i   thread (c, s) sums the rows i = s mod 8 of
//             column k0 + c, the eight partials meet in LDS in a fixed tree; then Ls[K, K]^T x_K = r_K as above.
// Every sum runs in an order that P alone decides.  A row with info != 0 gets NaN and nothing of it is read.
__global__ __launch_bounds__(256) void k_chol_solve(const double* __restrict__ L, const int P, const int ld,
                                                    const double* __restrict__ scale, const int* __restrict__ info,
                                                    const double* b, double* x)
{
    __shared__ double D[PGL_CH_NB][PGL_CH_PAD];
    __shared__ double part[8][PGL_CH_NB];
    __shared__ double xs[PGL_CH_NB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* Lm = L + (size_t)blockIdx.x * P * ld;
    const double* sc = scale + (size_t)blockIdx.x * P;
    const double* bv = b + (size_t)blockIdx.x * P;
    double* xv = x + (size_t)blockIdx.x * P;
    if (info[blockIdx.x] != 0) {                                 // (the whole workgroup, before any barrier)
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        for (int i = tid; i < P; i += 256) xv[i] = nan;
        return;
    }
    for (int i = tid; i < P; i += 256) xv[i] = bv[i] / sc[i];
    __syncthreads();
    // forward: Ls y = D^-1/2 b
    for (int k0 = 0; k0 < P; k0 += PGL_CH_NB) {
        const int nb = min(PGL_CH_NB, P - k0);
        for (int e = tid; e < PGL_CH_NB * PGL_CH_NB; e += 256) {
            const int i = e >> 5, c = e & 31;
            D[i][c] = (i < nb && c <= i) ? Lm[(size_t)(k0 + i) * ld + k0 + c] : (i == c ? 1.0 : 0.0);
        }
        for (int i = wave; i < nb; i += 4) {
            const double* row = Lm + (size_t)(k0 + i) * ld;
            double s = 0.0;
            for (int c = lane; c < k0; c += 64) s = fma(row[c], xv[c], s);
            for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
            if (lane == 0) xs[i] = xv[k0 + i] - s;
        }
        __syncthreads();
        if (wave == 0) {
            const int li = lane & 31;
            double yi = lane < nb ? xs[li] : 0.0;
            const double dii = D[li][li];
            for (int j = 0; j < nb; ++j) {
                const double yj = __shfl(yi / dii, j, 64);
                if (lane == j) yi = yj;
                else if (lane > j && lane < nb) yi = fma(-D[li][j], yj, yi);
            }
            if (lane < nb) xv[k0 + lane] = yi;
        }
        __syncthreads();
    }
    // backward: Ls^T z = y
    for (int k0 = ((P - 1) / PGL_CH_NB) * PGL_CH_NB; k0 >= 0; k0 -= PGL_CH_NB) {
        const int nb = min(PGL_CH_NB, P - k0);
        for (int e = tid; e < PGL_CH_NB * PGL_CH_NB; e += 256) {
            const int i = e >> 5, c = e & 31;
            D[i][c] = (i < nb && c <= i) ? Lm[(size_t)(k0 + i) * ld + k0 + c] : (i == c ? 1.0 : 0.0);
        }
        {
            // (rows below the block exist only when the block is a full one: k0 + c < P)
            const int c = tid & 31, s = tid >> 5;
            double a = 0.0;
            for (int i = k0 + PGL_CH_NB + s; i < P; i += 8) a = fma(Lm[(size_t)i * ld + k0 + c], xv[i], a);
            part[s][c] = a;
        }
        __syncthreads();
        if (wave == 0) {
            const int li = lane & 31;
            const double sum = ((part[0][li] + part[1][li]) + (part[2][li] + part[3][li])) +
                               ((part[4][li] + part[5][li]) + (part[6][li] + part[7][li]));
            double zi = lane < nb ? xv[k0 + li] - sum : 0.0;
            const double dii = D[li][li];
            for (int j = nb - 1; j >= 0; --j) {
                const double zj = __shfl(zi / dii, j, 64);
                if (lane == j) zi = zj;
                else if (lane < j) zi = fma(-D[j][li], zj, zi);
            }
            if (lane < nb) xv[k0 + lane] = zi;
        }
        __syncthreads();
    }
    for (int i = tid; i < P; i += 256) xv[i] = xv[i] / sc[i];
}

__global__ __launch_bounds__(256) void k_tri_inverse(double* __restrict__ L, const int P, const int ld,
                                                     const int* __restrict__ info)
{
    __shared__ double La[PGL_CH_NB][PGL_CH_PAD];
    __shared__ double Xb[PGL_CH_NB][PGL_CH_PAD];
    __shared__ double Ld[PGL_CH_NB][PGL_CH_PAD];
    __shared__ double Rs[PGL_CH_NB][PGL_CH_PAD];
    if (info[blockIdx.x] != 0) return;                           // (the whole workgroup, before any barrier)
    const int tid = threadIdx.x, ty = tid >> 4, tx = tid & 15;
    double* Lm = L + (size_t)blockIdx.x * P * ld;
    for (int J0 = 0; J0 < P; J0 += PGL_CH_NB) {
        for (int I0 = J0; I0 < P; I0 += PGL_CH_NB) {
            // R = delta_IJ - sum_{J <= K < I} Ls[I, K] X[K, J]: outputs (ty + 16 a, tx + 16 b) of the tile
            double r[2][2];
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) r[a][b] = (I0 == J0 && ty + 16 * a == tx + 16 * b) ? 1.0 : 0.0;
            for (int K0 = J0; K0 < I0; K0 += PGL_CH_NB) {
                // (K0 + 32 <= I0 < P and J0 + 32 <= I0: both tiles lie inside the matrix but for the rows of La past P;
                //  the block (J0, J0) holds X_JJ in its lower triangle and the caller's numbers above it)
                for (int e = tid; e < PGL_CH_NB * PGL_CH_NB; e += 256) {
                    const int i = e >> 5, c = e & 31;
                    La[i][c] = (I0 + i < P) ? Lm[(size_t)(I0 + i) * ld + K0 + c] : 0.0;
                    Xb[i][c] = (K0 > J0 || c <= i) ? Lm[(size_t)(K0 + i) * ld + J0 + c] : 0.0;
                }
                __syncthreads();
                for (int k = 0; k < PGL_CH_NB; ++k) {
                    const double a0 = La[ty][k], a1 = La[ty + 16][k], b0 = Xb[k][tx], b1 = Xb[k][tx + 16];
                    r[0][0] = fma(-a0, b0, r[0][0]);
                    r[0][1] = fma(-a0, b1, r[0][1]);
                    r[1][0] = fma(-a1, b0, r[1][0]);
                    r[1][1] = fma(-a1, b1, r[1][1]);
                }
                __syncthreads();
            }
            // the diagonal block Ls[I, I] (identity past P), and R into LDS
            for (int e = tid; e < PGL_CH_NB * PGL_CH_NB; e += 256) {
                const int i = e >> 5, c = e & 31;
                Ld[i][c] = (I0 + i < P) ? (c <= i ? Lm[(size_t)(I0 + i) * ld + I0 + c] : 0.0) : (c == i ? 1.0 : 0.0);
            }
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) Rs[ty + 16 * a][tx + 16 * b] = r[a][b];
            __syncthreads();
            if (tid < PGL_CH_NB) {                               // column tid of the tile: Ls[I, I] y = R[:, tid], in place
                for (int i = 0; i < PGL_CH_NB; ++i) {
                    double s = Rs[i][tid];
                    for (int l = 0; l < i; ++l) s = fma(-Ld[i][l], Rs[l][tid], s);
                    Rs[i][tid] = s / Ld[i][i];
                }
            }
            __syncthreads();
            for (int e = tid; e < PGL_CH_NB * PGL_CH_NB; e += 256) {
                const int i = e >> 5, c = e & 31;
                if (I0 + i < P && J0 + c <= I0 + i) Lm[(size_t)(I0 + i) * ld + J0 + c] = Rs[i][c];
            }
            __syncthreads();
        }
    }
}
