#include "at_launch.h"
/* packed local kernels for RAGGED batches: four groups of 16 lanes sweep a frame of K * 16 rows x l2 columns in which
 * every alignment keeps its own extents (at_sweep16.hip.h, RAG); pairs of similar size are put together by the host */
template <int K, bool PROF>
static at_sweep16_fn r3(int store, bool tb)
{
	if (!tb) return at::at_sweep16<at::K_LOCAL, 16, K, 4, true, true, false, true, AT_BITS16, 0, 0, PROF>;
	if (store == 0) return at::at_sweep16<at::K_LOCAL, 16, K, 4, true, true, true, true, AT_BITS16, 0, 0, PROF>;
	return at::at_sweep16<at::K_LOCAL, 16, K, 4, true, false, true, true, AT_BITS16, 0, 0, PROF>;
}
template <bool PROF>
static at_sweep16_fn r2(int k, int store, bool tb)
{
	switch (k) {
	case 4: return r3<4, PROF>(store, tb);
	case 5: return r3<5, PROF>(store, tb);
	case 6: return r3<6, PROF>(store, tb);
	case 7: return r3<7, PROF>(store, tb);
	case 10: return r3<10, PROF>(store, tb);
	case 13: return r3<13, PROF>(store, tb);
	default: return nullptr;
	}
}
at_sweep16_fn AT_NAME(at_pick16_rag_impl)(int kmode, int k, int store, bool tb)
{
	switch (kmode) {
	case at::K_LOCAL: return r2<false>(k, store, tb);
	AT_CASE_LOCAL_PROF(r2<true>(k, store, tb))
	default: return nullptr;
	}
}
