#include "at_launch.h"
/* packed kernels, one group of 64 lanes, K in 1..4 rows per lane, scores scaled by 16 (TS = 4) */
template <int MODE, int K, bool PROF = false>
static at_sweep16_fn p3(int store, bool tb)
{
	if (!tb) return store < 2 ? at::at_sweep16<MODE, 64, K, 4, true, true, false, false, AT_BITS16, 0, 0, PROF> : at::at_sweep16<MODE, 64, K, 4, false, false, false, false, AT_BITS16, 0, 0, PROF>;
	if (store == 0) return at::at_sweep16<MODE, 64, K, 4, true, true, true, false, AT_BITS16, 0, 0, PROF>;
	if (store == 1) return at::at_sweep16<MODE, 64, K, 4, true, false, true, false, AT_BITS16, 0, 0, PROF>;
	return at::at_sweep16<MODE, 64, K, 4, false, false, true, false, AT_BITS16, 0, 0, PROF>;
}
template <int MODE, bool PROF = false>
static at_sweep16_fn p2(int k, int store, bool tb)
{
	switch (k) {
	case 1: return p3<MODE, 1, PROF>(store, tb);
	case 2: return p3<MODE, 2, PROF>(store, tb);
	case 3: return p3<MODE, 3, PROF>(store, tb);
	default: return p3<MODE, 4, PROF>(store, tb);
	}
}
at_sweep16_fn AT_NAME(at_pick16_g64_ts4)(int kmode, int k, int store, bool tb)
{
	switch (kmode) {
	case at::K_GLOBAL: return p2<at::K_GLOBAL>(k, store, tb);
	case at::K_LOCAL: return p2<at::K_LOCAL>(k, store, tb);
	AT_CASE_LOCAL_PROF(p2<at::K_LOCAL, true>(k, store, tb))
	case at::K_FITJ: return p2<at::K_FITJ>(k, store, tb);
	default: return p2<at::K_FIT>(k, store, tb);
	}
}
