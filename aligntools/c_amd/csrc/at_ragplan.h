/*
 * at_ragplan.h -- the plan of a ragged batch on the host entry: the order in which the pairs are handed out and,
 * when the batch runs on the packed kernels in frames, its launches.  Pure arithmetic over the lengths: plain C++17, no HIP.
 */
#pragma once
#include "at_classes.h"
#include <algorithm>
#include <cstdint>
#include <vector>

namespace at {

struct RagLaunch {
	int64_t b0, b1;   /* order[b0 .. b1) */
	int g;            /* group width of the frames */
	int f1, f2;       /* the largest l1 and l2 of the launch */
};
struct RagPlan {
	std::vector<int> order;
	std::vector<RagLaunch> launches;   /* empty without frames: one launch over the whole order */
};

inline RagPlan rag_plan(int mode, bool overlap_tb, const int32_t *len1, const int32_t *len2, int64_t n, int max1, int max2,
                        int64_t min_bucket, bool frames)
{
	RagPlan p;
	std::vector<int> &order = p.order;
	auto cls = [&](int l1) { return rag_class(mode, overlap_tb, l1); };
	auto real = [&](size_t q) { return order[q] < 0 ? ~order[q] : order[q]; };   /* (a padding repeat is ~index) */
	if (!frames) {
		order.resize((size_t)n);
		for (int64_t k = 0; k < n; ++k) order[(size_t)k] = (int)k;
		std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return (int64_t)len1[x] * len2[x] > (int64_t)len1[y] * len2[y]; });
		return p;
	}
	/* both sorts are counting sorts over (major key, max2 - l2), stable in the index.  Local: the major key is the class, longest
	 * reads' first (a read's class never decreases with its length); the others: max1 - l1 */
	const bool local = mode == AT_MODE_LOCAL;
	std::vector<int> major((size_t)max1 + 1, 0);
	for (int l1 = 1; l1 <= max1; ++l1) major[(size_t)l1] = local ? major[(size_t)l1 - 1] + (l1 > 1 && cls(l1) != cls(l1 - 1)) : l1;
	const int top = major[(size_t)max1];
	const size_t span = (size_t)max2 + 1;
	auto key = [&](int64_t k) { return (size_t)(top - major[(size_t)len1[k]]) * span + (size_t)(max2 - len2[k]); };
	std::vector<int> start((size_t)(top + 1) * span + 1, 0);
	for (int64_t k = 0; k < n; ++k) ++start[key(k) + 1];
	for (size_t q = 1; q < start.size(); ++q) start[q] += start[q - 1];
	std::vector<int> sorted((size_t)n);
	for (int64_t k = 0; k < n; ++k) sorted[(size_t)start[key(k)]++] = (int)k;
	if (local) order.swap(sorted);
	else {
		for (size_t b0 = 0; b0 < sorted.size();) {
			size_t b1 = b0;
			const size_t run0 = order.size();
			while (b1 < sorted.size() && len1[sorted[b1]] == len1[sorted[b0]]) order.push_back(sorted[b1++]);
			const size_t per = (size_t)(2 * (64 / cls(len1[sorted[b0]]).g));
			while ((order.size() - run0) % per) order.push_back(~sorted[b1 - 1]);
			b0 = b1;
		}
	}
	for (size_t b0 = 0; b0 < order.size();) {
		const GroupRows c = cls(len1[real(b0)]);
		const int l2first = len2[real(b0)];
		RagLaunch L{(int64_t)b0, (int64_t)b0, c.g, 0, 0};
		for (size_t b1 = b0; b1 < order.size(); ++b1) {
			const int x = real(b1);
			if (cls(len1[x]) != c) break;
			if (local && (int64_t)(b1 - b0) >= min_bucket && (int64_t)len2[x] * 5 < (int64_t)l2first * 4) break;   /* more than 20 % narrower */
			L.f1 = std::max(L.f1, len1[x]); L.f2 = std::max(L.f2, len2[x]);
			L.b1 = (int64_t)b1 + 1;
		}
		p.launches.push_back(L);
		b0 = (size_t)L.b1;
	}
	return p;
}

}  // namespace at
