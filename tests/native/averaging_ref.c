/*
 * averaging_ref.c -- CPU restatement of the elastic-averaging and
 * Polyak-Ruppert barriers, for the tests only (tests/averaging_common.py
 * loads it; scripts/build_averaging_ref.sh builds it with gcc alone).
 *
 * Plain loops, one fmaf per cuBLAS saxpy element (y := fma (a, x, y)), in the
 * order of clib-multigpu/synch/synchronouseamsgd.c and synch/polyakruppert.c;
 * each line cites the reference line it restates.  Replica i lives on device
 * i % G (modelmanager.c:51-64).  With G > 1 every device accumulates its own
 * replicas and the partial sums are added in rank order starting from rank
 * 0's, which is the all-reduce the library's step uses; the reference chains
 * every replica into the default device's accumulator instead
 * (synchronouseamsgd.c:141-273, polyakruppert.c:177-290), so the two differ
 * in summation order.
 *
 * scratch holds (G + 1) * n floats.  Build with -ffp-contract=off.
 */
#include <math.h>
#include <stddef.h>
#include <string.h>

static int taken (int i, int g, int G, const int *locked, int first) {
	return i >= first && locked[i] && i % G == g;
}

/* acc[0..G) -> D, in rank order from rank 0's (synch/common.c:43-52) */
static void all_reduce (int G, size_t n, const float *acc, float *D) {
	size_t k;
	int g;
	memcpy (D, acc, n * sizeof (float));
	for (g = 1; g < G; ++g)
		for (k = 0; k < n; ++k)
			D[k] = D[k] + acc[(size_t) g * n + k];
}

/* Elastic averaging.  Reads and writes w; s is read only when G > 1; last
 * and the copy flags are not arguments: the step never looks at them. */
void cbr_elastic_average (int G, int size, size_t n, float alpha, float **z, float **s, float **w,
		const int *locked, int first, float *scratch) {
	float *D = scratch + (size_t) G * n;
	size_t k;
	int g, i;
	for (g = 0; g < G; ++g) {
		float *acc = scratch + (size_t) g * n;
		memset (acc, 0, n * sizeof (float));                                /* synchronouseamsgd.c:43, :141 */
		for (i = 0; i < size; ++i) {                                        /* :46-48 */
			if (! taken (i, g, G, locked, first))
				continue;
			const float *x = G > 1 ? s[i] : w[i];                           /* :55 (data), :184 (diff) */
			for (k = 0; k < n; ++k) {
				float d = fmaf (-1.0f, z[g][k], x[k]);                      /* :55-61 */
				w[i][k] = fmaf (-alpha, d, w[i][k]);                        /* :64-69 */
				acc[k] = fmaf (alpha, d, acc[k]);                           /* :72-77 */
			}
		}
	}
	all_reduce (G, n, scratch, D);
	for (g = 0; g < G; ++g)
		for (k = 0; k < n; ++k)
			z[g][k] = fmaf (1.0f, D[k], z[g][k]);                           /* :85-90 */
}

/* Polyak-Ruppert.  last[g] may be NULL (no momentum buffer).  Returns the
 * number of replicas that took z. */
int cbr_polyak_ruppert (int G, int size, size_t n, float alpha, int clock, float **z, float **last, float **w,
		const int *locked, int *copy, int first, float *scratch) {
	const float sf = 1. / (float) size;                                     /* polyakruppert.c:15 */
	const float raf = 1. / (float) (clock + 1);                             /* :16 */
	float *D = scratch + (size_t) G * n;
	size_t k;
	int g, i, copies = 0;
	for (g = 0; g < G; ++g) {
		float *acc = scratch + (size_t) g * n;
		memset (acc, 0, n * sizeof (float));                                /* :43 */
		for (i = 0; i < size; ++i) {                                        /* :46-48 */
			if (! taken (i, g, G, locked, first))
				continue;
			for (k = 0; k < n; ++k) {
				acc[k] = fmaf (sf, w[i][k], acc[k]);                        /* :51-56 */
				float d = fmaf (-1.0f, z[g][k], w[i][k]);                   /* :63-69 */
				if (alpha != 0)                                             /* :72 */
					w[i][k] = fmaf (-alpha, d, w[i][k]);                    /* :73-78 */
			}
		}
	}
	all_reduce (G, n, scratch, D);
	for (g = 0; g < G; ++g) {
		for (k = 0; k < n; ++k) {
			float L = fmaf (-1.0f, z[g][k], D[k]);                          /* :98-104 */
			if (last && last[g])
				last[g][k] = L;
			z[g][k] = fmaf (raf, L, z[g][k]);                               /* :107-112 */
		}
		for (i = 0; i < size; ++i) {                                        /* :122-124 */
			if (! taken (i, g, G, locked, first) || copy[i] <= 0)           /* :126 */
				continue;
			memcpy (w[i], z[g], n * sizeof (float));                        /* :129 */
			copy[i] = 0;                                                    /* :131 */
			++copies;
		}
	}
	return copies;
}
