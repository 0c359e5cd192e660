#include "at_launch.h"
/* packed kernels for RAGGED batches of reads of 209..304 bases: four groups of 16 lanes, 16 or 19 rows per lane -- global /
 * fit (work items of one read length) and local (frames that mix lengths) */
template <int MODE, int K, bool PROF = false>
static at_sweep16_fn x3(bool tb)
{
	if (!tb) return at::at_sweep16<MODE, 16, K, 4, true, true, false, true, AT_BITS16, 0, 0, PROF>;
	return at::at_sweep16<MODE, 16, K, 4, true, false, true, true, AT_BITS16, 0, 0, PROF>;
}
template <int MODE, bool PROF = false>
static at_sweep16_fn x2(int k, bool tb)
{
	switch (k) {
	case 16: return x3<MODE, 16, PROF>(tb);
	case 19: return x3<MODE, 19, PROF>(tb);
	default: return nullptr;
	}
}
at_sweep16_fn AT_NAME(at_pick16_rag16b)(int kmode, int k, int store, bool tb)
{
	if (tb && store != 1) return nullptr;
	switch (kmode) {
	case at::K_GLOBAL: return x2<at::K_GLOBAL>(k, tb);
	case at::K_LOCAL: return x2<at::K_LOCAL>(k, tb);
	AT_CASE_LOCAL_PROF(x2<at::K_LOCAL, true>(k, tb))
	case at::K_FITJ: return x2<at::K_FITJ>(k, tb);
	default: return x2<at::K_FIT>(k, tb);
	}
}
