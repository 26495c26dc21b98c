/* Host build of the argument rules of the segmented entry points (theano_pyglm_amd/csrc/pglm_gof.h) for
 * tests/test_gof_args_host.py:
 *   gof_args_count    pgl_gof_bad_count;  gof_args_offsets  pgl_gof_bad_offsets;
 *   gof_args_old_ks   the loop pgl_ks_uniform carried before the rules moved into the header, as it stood: 0 fine, 1 not;
 *   gof_args_table    vector k (0 <= k < GOF_ARGS_NTABLE) of the seeded table the test and the stand-alone program share:
 *                     writes *n + 1 <= GOF_ARGS_MAXN + 1 offsets and the answer pgl_gof_bad_offsets owes -- 0, or 1 + the
 *                     position of the planted fault (0: a negative first offset, p >= 1: off[p] < off[p - 1]).  Vectors 0 .. 8
 *                     have 8 segments and the fault at position k; of the rest one in four has none, and segments may be empty.
 * With -DGOF_ARGS_MAIN a stand-alone program (for a sanitizer build): the rules over the whole table, every vector in an
 * allocation of exactly its size, and the fixed cases of the test; exit status 0 and "ok" where all hold. */
#include <stdio.h>
#include <stdlib.h>
#include "../../theano_pyglm_amd/csrc/pglm_gof.h"

#define GOF_ARGS_NTABLE 200
#define GOF_ARGS_MAXN 40

int gof_args_count(long long M) { return pgl_gof_bad_count(M); }
long long gof_args_offsets(const long long* off, long long n) { return pgl_gof_bad_offsets(off, n); }

int gof_args_old_ks(const long long* off, long long M)
{
    for (long long m = 0; m < M; ++m)
        if (off[m + 1] < off[m] || off[0] < 0) return 1;
    return 0;
}

static unsigned long long mix(unsigned long long* s)       /* splitmix64 */
{
    unsigned long long z = (*s += 0x9e3779b97f4a7c15ULL);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
    return z ^ (z >> 31);
}

int gof_args_ntable(void) { return GOF_ARGS_NTABLE; }

void gof_args_table(int k, long long* off, long long* n, long long* want)
{
    unsigned long long s = 0x5eedULL + (unsigned long long)k;
    const long long len = k < 9 ? 8 : 1 + (long long)(mix(&s) % GOF_ARGS_MAXN);
    long long p = -1;                                       /* position of the fault; -1: none */
    if (k < 9) p = k;
    else if (k % 4) p = (long long)(mix(&s) % (unsigned long long)(len + 1));
    off[0] = 0;
    for (long long i = 1; i <= len; ++i) off[i] = off[i - 1] + (long long)(mix(&s) % 5);    /* (0: an empty segment) */
    if (p == 0) off[0] = -1 - (long long)(mix(&s) % 3);
    if (p > 0) off[p] = off[p - 1] - 1 - (long long)(mix(&s) % 3);
    *n = len;
    *want = p < 0 ? 0 : 1 + p;
}

#ifdef GOF_ARGS_MAIN
#define CHECK(cond)                                                 \
    do {                                                            \
        if (!(cond)) {                                              \
            printf("line %d: %s does not hold\n", __LINE__, #cond); \
            return 1;                                               \
        }                                                           \
    } while (0)

int main(void)
{
    long long faults = 0;
    for (int k = 0; k < GOF_ARGS_NTABLE; ++k) {
        long long buf[GOF_ARGS_MAXN + 1], n, want;
        gof_args_table(k, buf, &n, &want);
        long long* off = (long long*)malloc((size_t)(n + 1) * sizeof(long long));
        CHECK(off != NULL);
        for (long long i = 0; i <= n; ++i) off[i] = buf[i];
        CHECK(pgl_gof_bad_offsets(off, n) == want);
        CHECK(gof_args_old_ks(off, n) == (want != 0));
        faults += want != 0;
        free(off);
    }
    CHECK(faults > 100 && faults < GOF_ARGS_NTABLE);
    const long long empty[4] = {0, 0, 0, 0}, one[2] = {0, 5}, neg[3] = {-1, 0, 3}, first[4] = {2, 1, 3, 4},
                    middle[5] = {0, 2, 4, 3, 9}, last[4] = {0, 1, 5, 4};
    CHECK(pgl_gof_bad_offsets(empty, 3) == 0 && pgl_gof_bad_offsets(one, 1) == 0 && pgl_gof_bad_offsets(neg, 2) == 1);
    CHECK(pgl_gof_bad_offsets(first, 3) == 2 && pgl_gof_bad_offsets(middle, 4) == 4 && pgl_gof_bad_offsets(last, 3) == 4);
    CHECK(pgl_gof_bad_count(0) == 1 && pgl_gof_bad_count(1) == 0 && pgl_gof_bad_count(-1) == 1);
    CHECK(pgl_gof_bad_count(0x7fffffffLL) == 0 && pgl_gof_bad_count(0x80000000LL) == 1);
    printf("ok: %d vectors, %lld with a fault\n", GOF_ARGS_NTABLE, faults);
    return 0;
}
#endif
