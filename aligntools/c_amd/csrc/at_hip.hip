/*
 * at_hip.hip -- the C-ABI shim (include/aligntools_hip.h) over the gfx950
 * sweep kernel (at_sweep.hip.h).  Host C++ here is plumbing only: argument
 * checks, packing, the choice of storage class, launches.  There is no CPU
 * compute path: every DP cell is computed on the GPU or the call fails.
 */
#include "at_launch.h"
#include "at_classes.h"
#include "at_ragplan.h"
#include "at_queryplan.h"
#include "at_pack.hip.h"
#include "at_render.hip.h"
#include "at_myers.hip.h"
#include "at_search.hip.h"
#include "at_revcomp.hip.h"
#include "at_cigar.hip.h"
#include "at_edit_tb.hip.h"
#include "at_infix.hip.h"
#include "at_scan.hip.h"
#include "at_scanhits.hip.h"
#include "at_tilescan.hip.h"
#include "at_pairhits.hip.h"
#include "../../../include/aligntools_hip.h"

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <numeric>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <thread>
#include <vector>

#ifndef AT_DIAG_SWEEP_ONLY
#define AT_DIAG_SWEEP_ONLY 0   /* 1: a throw-away build in which AT_DIAG_NO_WALK_KERNEL=1 skips pass 2 (tools/gpu/profiles.sh, through tools/ab_lib.sh) */
#endif

using at::SweepArgs;
using at::Sweep16Args;

/* The host entry's helper threads: chunk c of a batch runs on worker c (chunk 0 on the caller's thread).  They live as long as the
 * handle -- starting five threads per call was a tenth of a millisecond before any byte moved. */
struct HostPool {
	std::vector<std::thread> th;
	std::mutex mu;
	std::condition_variable cv_go, cv_done;
	std::function<void(int)> job;
	unsigned long long gen = 0;
	int active = 0, pending = 0;
	bool stop = false;
	void worker(int w)
	{
		unsigned long long seen = 0;
		for (;;) {
			std::function<void(int)> fn;
			{
				std::unique_lock<std::mutex> lk(mu);
				cv_go.wait(lk, [&] { return stop || gen != seen; });
				if (stop) return;
				seen = gen;
				if (w >= active) continue;
				fn = job;
			}
			fn(w);
			{
				std::lock_guard<std::mutex> lk(mu);
				if (--pending == 0) cv_done.notify_all();
			}
		}
	}
	/* run fn(1) .. fn(n - 1) on the workers and fn(0) here; returns when all are done */
	void run(int n, const std::function<void(int)> &fn)
	{
		while ((int)th.size() < n - 1) { const int w = (int)th.size() + 1; th.emplace_back([this, w] { worker(w); }); }
		{
			std::lock_guard<std::mutex> lk(mu);
			job = fn; active = n; pending = n - 1; ++gen;
		}
		cv_go.notify_all();
		fn(0);
		std::unique_lock<std::mutex> lk(mu);
		cv_done.wait(lk, [&] { return pending == 0; });
	}
	~HostPool()
	{
		{ std::lock_guard<std::mutex> lk(mu); stop = true; }
		cv_go.notify_all();
		for (auto &t : th) t.join();
	}
};

struct at_handle {
	int device = 0;
	int ncu = 256;
	size_t lds_per_cu = 160 * 1024;
	hipStream_t stream = nullptr;   /* used by the host-buffer entry */
	/* scoring */
	int m = 1, u = -2, o = -5, e = -1, j = -10, use_jump = 0;
	std::vector<int> sites;
	int min_on = 0, min_score = 0;  /* at_set_min_score: all-vs-all overlap scores skip pairs proven below it */
	int edit_tb = 0;                /* at_set_edit_traceback: edit batches with want_traceback deliver their ops (at_edit_tb.hip.h) */
	int edit_infix = 0;             /* at_set_edit_infix: AT_MODE_EDIT is the best match of s1 inside s2 (at_infix.hip.h) */
	/* device scratch (grow-only) */
	uint32_t *d_sitemask = nullptr; size_t sitemask_words = 0; int sitemask_for_l2 = -1; bool sitemask_dirty = true;
	/* the site mask's way up: page-locked buffers used in turn, each with the event behind its copy (ensure_sitemask) */
	struct SiteStage { void *host = nullptr; size_t bytes = 0; hipEvent_t done = nullptr; };
	std::vector<SiteStage> site_stage;
	unsigned site_next = 0;
	uint32_t *d_ws = nullptr; size_t ws_bytes = 0;
	uint32_t *d_ck = nullptr; size_t ck_bytes = 0;   /* two-pass tracebacks with a walk kernel: a launch's checkpoints */
	bool ck_alloc_failed = false;                    /* ... could not be allocated once: this handle keeps to the rounds inside the sweep's kernel
	                                                  * for the rest of its life (a later batch would only meet the same shortage) */
	unsigned long long *d_queue = nullptr;
	int last_span = 0;              /* max_len1 + max_len2 of the handle's latest batch: the rendering kernel's hint for its group width */
	void *d_in = nullptr; size_t in_bytes = 0;
	void *d_out = nullptr; size_t out_bytes = 0;
	void *d_desc = nullptr; size_t desc_bytes = 0;
	void *d_order = nullptr; size_t order_bytes = 0;
	void *d_str = nullptr; size_t str_bytes = 0;
	void *d_scan = nullptr; size_t scan_bytes = 0;
	void *d_cand = nullptr; size_t cand_bytes = 0;       /* at_scan_hits: a slice's candidates and what the selection makes of them */
	void *d_sorttmp = nullptr; size_t sorttmp_bytes = 0; /* ... the radix sort's scratch */
	int *d_rflag = nullptr;         /* at_render_k's "op list walks off its sequences" flag */
	/* host entry: page-locked staging -- descriptor block, raw bytes on their way up, results and payload on their way down */
	void *hp_desc = nullptr; size_t hp_desc_bytes = 0;
	void *hp_blob = nullptr; size_t hp_blob_bytes = 0;
	void *hp_out = nullptr; size_t hp_out_bytes = 0;
	void *hp_flag = nullptr;
	void *hp_order = nullptr; size_t hp_order_bytes = 0;   /* the processing order of a ragged batch */
	double last_payload_per_pair = 16.0;   /* traceback bytes per pair of the latest batch: how much payload the next one fetches unasked */
	/* all-vs-all in slices: a copy stream, pinned result buffers (two sets, used in turn) and their events */
	hipStream_t copy_stream = nullptr;
	void *h_pin = nullptr; size_t pin_bytes = 0;
	hipEvent_t ev_sweep[2] = {nullptr, nullptr}, ev_copy[2] = {nullptr, nullptr};
	std::vector<at_handle *> kids;  /* helper handles of the host entry: chunks of one batch in flight side by side */
	HostPool *pool = nullptr;       /* ... and the threads they run on */
	void *comm = nullptr;           /* multi-process batches: the communicator (at_comm.hip) */
	char err[512] = {0};
	char cfg[640] = "none";
	int last_render_lanes = 0;      /* lanes per pair of the latest at_render_batch_device (at_last_config of the host entry's strings) */
	/* the host entry's CIGAR form: device block (counts, statistics, words), its page-locked mirror, and what a chunk leaves for the
	 * parent to lay into the caller's buffer behind the join */
	void *d_cg = nullptr; size_t cg_bytes = 0;
	void *hp_cg = nullptr; size_t hp_cg_bytes = 0;
	const uint32_t *cg_words = nullptr; int64_t cg_total = 0;
	double last_cigar_per_pair = 4.0;      /* CIGAR words per pair of the latest batch: how many the next one fetches unasked */
	int last_cigar_lanes = 0;       /* lanes per pair of the latest at_cigar_batch_device */
};

static thread_local char g_err[512] = "no error";   /* per thread: the host entry runs chunks on helper threads */

static int fail(at_handle *h, int code, const char *fmt, ...)
{
	char buf[512];
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(buf, sizeof buf, fmt, ap);
	va_end(ap);
	snprintf(g_err, sizeof g_err, "%s", buf);
	if (h) snprintf(h->err, sizeof h->err, "%s", buf);
	return code;
}

/* at_last_config grows by notes: what a later stage of the call did */
__attribute__((format(printf, 2, 3))) static void cfg_append(at_handle *h, const char *fmt, ...)
{
	const size_t used = strlen(h->cfg);
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(h->cfg + used, sizeof h->cfg - used, fmt, ap);
	va_end(ap);
}

/* no C++ exception crosses the C ABI (std::bad_alloc from a vector or a string on the host side): it becomes an error code */
template <typename F>
static int guarded(at_handle *h, const char *who, F &&body)
{
	try { return body(); }
	catch (const std::bad_alloc &) { return fail(h, AT_ERR_NOMEM, "%s: out of host memory", who); }
	catch (const std::exception &ex) { return fail(h, AT_ERR_NOMEM, "%s: %s", who, ex.what()); }
	catch (...) { return fail(h, AT_ERR_NOMEM, "%s: unknown C++ exception", who); }
}

/* (a failed call's error is also the thread's last error: read away, so that the failure is reported once, by our return code) */
#define HIP_TRY(h, call)                                                                      \
	do {                                                                                      \
		hipError_t e_ = (call);                                                               \
		if (e_ != hipSuccess) {                                                               \
			(void)hipGetLastError();                                                          \
			return fail((h), AT_ERR_NODEVICE, "%s: %s", #call, hipGetErrorString(e_));        \
		}                                                                                     \
	} while (0)

/* The runtime keeps a failed call's error as the thread's last error until somebody reads it, and the check behind a launch
 * (HIP_TRY(h, hipGetLastError())) would report such a leftover -- of an earlier call, ours or the caller's -- as the launch's own:
 * every entry that launches reads it away first */
static inline void drop_stale_error() { (void)hipGetLastError(); }

extern "C" const char *at_last_error(const at_handle *h) { return h ? h->err : g_err; }
extern "C" const char *at_last_config(const at_handle *h) { return h ? h->cfg : "none"; }
/* diagnostic builds (-DAT_TP_STATS=1): the 8 words of the handle's work counter block, after a device synchronisation */
extern "C" int at_debug_counters(at_handle *h, unsigned long long *out8)
{
	if (!h || !out8 || !h->d_queue) return AT_ERR_ARG;
	if (hipDeviceSynchronize() != hipSuccess) return AT_ERR_NODEVICE;
	return hipMemcpy(out8, h->d_queue, 64, hipMemcpyDeviceToHost) == hipSuccess ? AT_OK : AT_ERR_NODEVICE;
}

extern "C" int at_init(const int *device_ids, int n_devices, at_handle **out)
{
	if (!out) return fail(nullptr, AT_ERR_ARG, "at_init: out is NULL");
	*out = nullptr;
	if (n_devices != 1 && !(n_devices == 0 && !device_ids))
		return fail(nullptr, AT_ERR_ARG, "at_init: one process per GPU -- n_devices must be 1 (got %d)", n_devices);
	int count = 0;
	hipError_t e = hipGetDeviceCount(&count);
	if (e != hipSuccess || count <= 0)
		return fail(nullptr, AT_ERR_NODEVICE, "at_init: no HIP device (%s); there is no CPU fallback",
		            e == hipSuccess ? "device count 0" : hipGetErrorString(e));
	int dev = 0;
	if (device_ids) dev = device_ids[0];
	else if (hipGetDevice(&dev) != hipSuccess) dev = 0;
	if (dev < 0 || dev >= count) return fail(nullptr, AT_ERR_ARG, "at_init: device %d out of range (0..%d)", dev, count - 1);
	at_handle *h = new at_handle();
	h->device = dev;
	/* a failing step frees what the earlier ones made: the caller gets no handle to destroy */
	auto init = [&]() -> int {
		HIP_TRY(h, hipSetDevice(dev));
		hipDeviceProp_t prop;
		HIP_TRY(h, hipGetDeviceProperties(&prop, dev));
		h->ncu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
		if (prop.maxSharedMemoryPerMultiProcessor > 0) h->lds_per_cu = prop.maxSharedMemoryPerMultiProcessor;
		HIP_TRY(h, hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
		HIP_TRY(h, hipMalloc((void **)&h->d_rflag, 256));
		HIP_TRY(h, hipMemset(h->d_rflag, 0, 256));
		HIP_TRY(h, hipHostMalloc(&h->hp_flag, 256, hipHostMallocDefault));
		return AT_OK;
	};
	const int rc = init();
	if (rc != AT_OK) { at_destroy(h); return rc; }   /* (the message is in the calling thread's at_last_error(NULL)) */
	h->err[0] = 0;
	*out = h;
	return AT_OK;
}

extern "C" void at_comm_destroy(at_handle *h);
/* what at_comm.hip needs of a handle */
extern "C" int at_handle_device(const at_handle *h) { return h->device; }
extern "C" int at_comm_fail(at_handle *h, int code, const char *msg) { return fail(h, code, "%s", msg); }
extern "C" void **at_comm_slot(at_handle *h) { return &h->comm; }
extern "C" void at_get_scoring(const at_handle *h, int *v7, const int **sites)
{
	v7[0] = h->m; v7[1] = h->u; v7[2] = h->o; v7[3] = h->e; v7[4] = h->j; v7[5] = h->use_jump; v7[6] = (int)h->sites.size();
	*sites = h->sites.data();
}

extern "C" void at_destroy(at_handle *h)
{
	if (!h) return;
	if (h->comm) at_comm_destroy(h);
	delete h->pool; h->pool = nullptr;      /* (joins its threads) */
	for (at_handle *k : h->kids) at_destroy(k);
	h->kids.clear();
	(void)hipSetDevice(h->device);
	if (h->d_sitemask) (void)hipFree(h->d_sitemask);
	for (at_handle::SiteStage &c : h->site_stage) {
		if (c.done) (void)hipEventDestroy(c.done);
		if (c.host) (void)hipHostFree(c.host);
	}
	if (h->d_ws) (void)hipFree(h->d_ws);
	if (h->d_ck) (void)hipFree(h->d_ck);
	if (h->d_queue) (void)hipFree(h->d_queue);
	if (h->d_in) (void)hipFree(h->d_in);
	if (h->d_out) (void)hipFree(h->d_out);
	if (h->d_desc) (void)hipFree(h->d_desc);
	if (h->d_order) (void)hipFree(h->d_order);
	if (h->d_str) (void)hipFree(h->d_str);
	if (h->d_scan) (void)hipFree(h->d_scan);
	if (h->d_cand) (void)hipFree(h->d_cand);
	if (h->d_sorttmp) (void)hipFree(h->d_sorttmp);
	if (h->d_rflag) (void)hipFree(h->d_rflag);
	if (h->d_cg) (void)hipFree(h->d_cg);
	if (h->hp_cg) (void)hipHostFree(h->hp_cg);
	if (h->h_pin) (void)hipHostFree(h->h_pin);
	if (h->hp_desc) (void)hipHostFree(h->hp_desc);
	if (h->hp_blob) (void)hipHostFree(h->hp_blob);
	if (h->hp_out) (void)hipHostFree(h->hp_out);
	if (h->hp_flag) (void)hipHostFree(h->hp_flag);
	if (h->hp_order) (void)hipHostFree(h->hp_order);
	for (int q = 0; q < 2; ++q) {
		if (h->ev_sweep[q]) (void)hipEventDestroy(h->ev_sweep[q]);
		if (h->ev_copy[q]) (void)hipEventDestroy(h->ev_copy[q]);
	}
	if (h->copy_stream) (void)hipStreamDestroy(h->copy_stream);
	if (h->stream) (void)hipStreamDestroy(h->stream);
	delete h;
}

extern "C" int at_set_min_score(at_handle *h, int enabled, int32_t min_score)
{
	if (!h) return fail(nullptr, AT_ERR_ARG, "at_set_min_score: NULL handle");
	h->min_on = enabled ? 1 : 0;
	h->min_score = min_score;
	return AT_OK;
}

extern "C" int at_set_edit_traceback(at_handle *h, int enabled)
{
	if (!h) return fail(nullptr, AT_ERR_ARG, "at_set_edit_traceback: NULL handle");
	h->edit_tb = enabled ? 1 : 0;
	return AT_OK;
}

extern "C" int at_set_edit_infix(at_handle *h, int enabled)
{
	if (!h) return fail(nullptr, AT_ERR_ARG, "at_set_edit_infix: NULL handle");
	h->edit_infix = enabled ? 1 : 0;
	return AT_OK;
}

extern "C" int at_set_scoring(at_handle *h, int m, int u, int o, int e, int j, int use_jump, const int *sites, int nsites)
{
	if (!h) return fail(nullptr, AT_ERR_ARG, "at_set_scoring: NULL handle");
	if (nsites < 0 || (nsites > 0 && !sites)) return fail(h, AT_ERR_ARG, "at_set_scoring: bad site list");
	h->m = m; h->u = u; h->o = o; h->e = e; h->j = j; h->use_jump = use_jump ? 1 : 0;
	h->sites.assign(sites, sites + nsites);
	h->sitemask_dirty = true;
	return AT_OK;
}

/* ------------------------------------------------------------------ packing */

static inline int code2(uint8_t c)
{
	switch (c) { case 'A': return 0; case 'C': return 1; case 'G': return 2; case 'T': return 3; default: return -1; }
}

extern "C" int64_t at_pack_words(int64_t npairs, const int32_t *len1, const int32_t *len2, int bits)
{
	if (npairs < 0 || !len1 || !len2 || (bits != 2 && bits != 8)) return -1;
	const int bpw = 32 / bits;
	int64_t w = 0;
	for (int64_t k = 0; k < npairs; ++k) {
		if (len1[k] < 0 || len2[k] < 0) return -1;
		w += (len1[k] + bpw - 1) / bpw + 1 + (len2[k] + bpw - 1) / bpw + 1;   /* +1: the window reads one word ahead */
	}
	return w + 4;
}

static void pack_one(const uint8_t *s, int len, int bits, uint32_t *dst)
{
	const int bpw = 32 / bits;
	const int nw = (len + bpw - 1) / bpw + 1;
	for (int w = 0; w < nw; ++w) {
		uint32_t v = 0;
		for (int b = 0; b < bpw; ++b) {
			const int idx = w * bpw + b;
			if (idx >= len) break;
			const uint32_t c = bits == 2 ? (uint32_t)code2(s[idx]) : (uint32_t)s[idx];
			v |= c << (b * bits);
		}
		dst[w] = v;
	}
}

extern "C" int at_pack_batch(int64_t npairs, const uint8_t *seq_blob,
                             const int64_t *off1, const int32_t *len1, const int64_t *off2, const int32_t *len2,
                             int bits, int *bits_out, uint32_t *words_out, int64_t *woff1_out, int64_t *woff2_out)
{
	if (npairs < 0 || !seq_blob || !off1 || !len1 || !off2 || !len2 || !woff1_out || !woff2_out)
		return fail(nullptr, AT_ERR_ARG, "at_pack_batch: NULL argument");
	if (bits == 0) {
		bits = 2;
		for (int64_t k = 0; k < npairs && bits == 2; ++k) {
			const uint8_t *a = seq_blob + off1[k], *b = seq_blob + off2[k];
			for (int x = 0; x < len1[k]; ++x) if (code2(a[x]) < 0) { bits = 8; break; }
			for (int x = 0; x < len2[k] && bits == 2; ++x) if (code2(b[x]) < 0) { bits = 8; break; }
		}
	}
	if (bits != 2 && bits != 8) return fail(nullptr, AT_ERR_ARG, "at_pack_batch: bits must be 0, 2 or 8");
	if (bits == 2) {   /* a caller that forces 2-bit words must hand over pure ACGT: there is no code for anything else */
		for (int64_t k = 0; k < npairs; ++k) {
			const uint8_t *a = seq_blob + off1[k], *b = seq_blob + off2[k];
			for (int x = 0; x < len1[k]; ++x) if (code2(a[x]) < 0) return fail(nullptr, AT_ERR_ARG, "at_pack_batch: pair %lld: byte 0x%02x cannot be packed in 2 bits", (long long)k, a[x]);
			for (int x = 0; x < len2[k]; ++x) if (code2(b[x]) < 0) return fail(nullptr, AT_ERR_ARG, "at_pack_batch: pair %lld: byte 0x%02x cannot be packed in 2 bits", (long long)k, b[x]);
		}
	}
	if (bits_out) *bits_out = bits;
	if (!words_out) return AT_OK;   /* query only */
	const int bpw = 32 / bits;
	int64_t w = 0;
	for (int64_t k = 0; k < npairs; ++k) {
		woff1_out[k] = w;
		pack_one(seq_blob + off1[k], len1[k], bits, words_out + w);
		w += (len1[k] + bpw - 1) / bpw + 1;
		woff2_out[k] = w;
		pack_one(seq_blob + off2[k], len2[k], bits, words_out + w);
		w += (len2[k] + bpw - 1) / bpw + 1;
	}
	for (int x = 0; x < 4; ++x) words_out[w + x] = 0;
	return AT_OK;
}

extern "C" int at_render(const uint8_t *ops, int32_t nops, const uint8_t *s1, int32_t end_i,
                         const uint8_t *s2, int32_t end_j, char *r1, char *r2)
{
	if (nops < 0 || !r1 || !r2 || (nops > 0 && (!ops || !s1 || !s2))) return AT_ERR_ARG;
	int i = end_i, j = end_j;
	for (int k = 0; k < nops; ++k) {
		const int pos = nops - 1 - k;
		switch (ops[k]) {
		case AT_OP_MID: if (i <= 0 || j <= 0) return AT_ERR_ARG; r1[pos] = (char)s1[--i]; r2[pos] = (char)s2[--j]; break;
		case AT_OP_LOW: if (i <= 0) return AT_ERR_ARG; r1[pos] = (char)s1[--i]; r2[pos] = '-'; break;
		case AT_OP_UPP:
		case AT_OP_JUMP: if (j <= 0) return AT_ERR_ARG; r1[pos] = '-'; r2[pos] = (char)s2[--j]; break;
		default: return AT_ERR_ARG;
		}
	}
	r1[nops] = 0; r2[nops] = 0;
	return AT_OK;
}

/* the CIGAR rule of include/aligntools_hip.h, one op at a time; the kernel (at_cigar.hip) computes the same from ballots */
extern "C" int at_cigar(const uint8_t *ops, int32_t nops, const uint8_t *s1, int32_t end_i,
                        const uint8_t *s2, int32_t end_j, int flags, uint32_t *cigar, int32_t *ncigar, int32_t stats[8])
{
	if (nops < 0 || end_i < 0 || end_j < 0 || !ncigar || !stats || (nops > 0 && (!ops || !s1 || !s2))) return AT_ERR_ARG;
	const bool merge = (flags & AT_CIGAR_M) != 0;
	/* two walks, as on the device: the first counts and checks, the second writes run r (from the END) to cigar[runs - 1 - r] */
	int runs = 0;
	for (int pass = 0; pass < 2; ++pass) {
		int i = end_i, j = end_j, r = 0, cur = -1, len = 0;
		int32_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
		bool bad = false;
		for (int k = 0; k < nops && !bad; ++k) {
			int cls = -1;
			switch (ops[k]) {
			case AT_OP_MID: if (i <= 0 || j <= 0) { bad = true; break; } --i; --j; cls = s1[i] == s2[j] ? 7 : 8; ++st[cls == 7 ? AT_CG_EQUAL : AT_CG_UNEQUAL]; break;
			case AT_OP_LOW: if (i <= 0) { bad = true; break; } --i; cls = 1; ++st[AT_CG_INS]; break;
			case AT_OP_UPP: if (j <= 0) { bad = true; break; } --j; cls = 2; ++st[AT_CG_DEL]; break;
			case AT_OP_JUMP: if (j <= 0) { bad = true; break; } --j; cls = 3; ++st[AT_CG_SKIP]; break;
			default: bad = true; break;
			}
			if (bad) break;
			const int rc = merge && cls >= 7 ? 0 : cls;
			if (rc != cur) {
				if (pass == 1 && cur >= 0) cigar[runs - r] = ((uint32_t)len << 4) | (uint32_t)cur;
				if (cls == 1 || cls == 2) ++st[AT_CG_GAPS];
				cur = rc; len = 0; ++r;
			}
			++len;
		}
		if (bad) {
			*ncigar = -1;
			for (int q = 0; q < 8; ++q) stats[q] = -1;
			return AT_ERR_DOMAIN;
		}
		if (pass == 1 && cur >= 0) cigar[runs - r] = ((uint32_t)len << 4) | (uint32_t)cur;
		st[AT_CG_START_I] = i; st[AT_CG_START_J] = j;
		runs = r;
		memcpy(stats, st, sizeof st);
		*ncigar = runs;
		if (!cigar) break;
	}
	return AT_OK;
}

/* ----------------------------------------------------------------- dispatch */

static long long env_ll(const char *name, long long dflt)
{
	const char *v = getenv(name);
	return v && *v ? atoll(v) : dflt;
}

struct Layout {
	int off_bound, off_ptr, off_sm, nsm, k, ptr_lanes;
	long long words;
};

/* rows per lane: enough to hold max_l1 in one strip of 64 lanes, at most 4 */
static int rows_per_lane(int max_l1, bool deep = false)
{
	const long long forced = getenv("AT_ROWS_PER_LANE") ? atoll(getenv("AT_ROWS_PER_LANE")) : 0;
	if (forced >= 1 && forced <= 4) return (int)forced;
	const int need = std::max(1, (max_l1 + 63) / 64);
	/* single-state kernels without a pointer matrix (overlap scores, edit) hold one value per row: 8 or 16 rows per
	 * lane spread the per-step work (shuffles, end-cell scan, loop) over more cells and fit 1 kbp in one strip */
	if (deep && need > 4 && !(forced == 8 || forced == 16)) return need <= 8 ? 8 : 16;
	if (deep && (forced == 8 || forced == 16)) return (int)forced;
	return std::min(4, need);
}

static Layout layout_for(int kmode, int bits, bool tb, int max_l1, int max_l2)
{
	const int bpw = 32 / bits;
	const int tbk = (max_l2 + 63 + at::kBlk - 1) / at::kBlk;
	const int rpb = kmode == at::K_FITJ ? 2 : 1;
	Layout L;
	L.k = rows_per_lane(max_l1, (kmode == at::K_OVERLAP && !tb) || kmode == at::K_EDIT);
	L.ptr_lanes = std::max(1, std::min(64, (max_l1 + L.k - 1) / L.k));
	const long long nstrips = (max_l1 + 64 * L.k - 1) / (64 * L.k);
	(void)bpw;
	long long nref = (at::kPad + (long long)tbk * at::kBlk) / 4 + 4;   /* s2 staged one byte per base */
	nref = (nref + 1) & ~1LL;
	const long long nbound = 2LL * (max_l2 + 2);
	const long long nptr = (tb && kmode != at::K_EDIT) ? nstrips * tbk * rpb * L.k * L.ptr_lanes + 64 : 0;
	const long long nsm = kmode == at::K_FITJ ? (((long long)max_l2 + 64 + 64 + 128 + 31) / 32 + 2 + 1) & ~1LL : 0;
	L.off_bound = (int)nref;
	L.off_sm = (int)(nref + nbound);
	L.nsm = (int)nsm;
	L.off_ptr = (int)(nref + nbound + nsm);
	L.words = nref + nbound + nsm + nptr;
	return L;
}

/* The 2-bit kernels read scores from a signed-byte LUT: scaled match/mismatch (minus the gap for overlap) must fit. */
static bool scores_fit_byte(const at_handle *h, int mode)
{
	long long a, b, c = 0, d = 0;
	if (mode == AT_MODE_EDIT) { a = 0; b = h->u; c = (long long)h->u - 2; }   /* (the sweep's table holds cost - 2: at_sweep.hip.h, RAMP) */
	else if (mode == AT_MODE_OVERLAP) {
		a = 16LL * (h->m - h->o); b = 16LL * (h->u - h->o);                     /* with pointers: s - o, scaled */
		c = (long long)h->m - 2LL * h->o; d = (long long)h->u - 2LL * h->o;     /* scores only: s - 2 o, unscaled */
	} else { a = 16LL * h->m; b = 16LL * h->u; }
	return std::llabs(a) <= 127 && std::llabs(b) <= 127 && std::llabs(c) <= 127 && std::llabs(d) <= 127;
}

/* ---- packed int16 path (at_sweep16.hip.h): two same-shape pairs per wave ---- */
struct Layout16 {
	int off_refb, off_bound, off_ptr, off_sm, nsm, g, k, ptr_lanes;
	long long words;
};

/* Group width: reads of up to 152 bases run as 8 groups of 8 lanes x K rows (16 alignments per wave: 94 % of the
 * lane-steps inside a 150 x 150 matrix, the per-step overhead spread over 19 rows; reads of up to 76 bases: 16 groups of 4
 * lanes, 32 alignments per wave), up to 208 bases as 4 groups of 16
 * lanes (8 alignments per wave, 85 %; one group of 64 lanes: 59 %) and so do 209..304 bases with 16 / 19 rows per lane,
 * 305..608 bases as 2 groups of 32 lanes (10 .. 19 rows per lane), everything
 * else as one group of 64 lanes.  AT_GROUP = 8 / 16 / 32 / 64 caps the choice (A/B runs); ragged frames name their group width themselves. */
/* The 8-lane groups x 19 rows (reads of 129 .. 152 bases): which batches take the two-pass kernels with the walk kernel by default --
 * fit (with or without -s) against a second sequence at least one and a half times as long: the sweep is long against the walkers' chain
 * of rounds (150-base reads, launches in flight / one at a time against the one-pass kernels, -s / without: l2 = 160 +12 % / -2 %, +7 % /
 * -3 %; l2 = 225 +13 % / +4 %, +8 % / +7 %; l2 = 300 +12 % / +10 %, +12 % / +11 %; l2 = 400 +12 % / +14 %, +16 % / +17 %; r05n)
 * (same box, launches in flight / one at a time: C4 150 x 500 -s 2 210 -> 2 380 / 1 960 -> 2 180 GCUPS, the same without -s 3 150 -> 3 750 /
 * 2 590 -> 3 350).  Global and local 150 x 150 gain with launches in flight (2 470 -> 2 700, 3 050 -> 3 180) and lose alone (2 380 ->
 * 2 230, 2 800 -> 2 490): AT_TWO_PASS=2 AT_TP_SPLIT=1 asks for them. */
static bool tp_split_narrow_default(int kmode, int l1, int l2) { return (kmode == at::K_FITJ || kmode == at::K_FIT) && 2LL * l2 >= 3LL * l1; }
static Layout16 layout16_for(bool tb, bool hasj, int l1, int l2, int ts, int force_g = 0, bool overlap = false, int kmode = -1, int force_k = 0, int two_pass = 0)   /* two_pass: 1 = the rounds inside the sweep's kernel (its staging area and walkers' tiles in LDS), 2 = a walk kernel; force_g: 8 / 16 = ragged frames on that group width; 64 = the 64-lane items behind a batch of narrow-group items, force_k rows per lane */
{
	Layout16 L;
	const long long g_forced = env_ll("AT_GROUP", 0);
	L.g = 64;
	L.k = rows_per_lane(l1);
	/* scores only, scores x4: 16 rows per lane (strips of 1 024 rows) once that is fewer lane-steps than strips of 256 --
	 * per step a lane does 16 x 11 + 25 instructions instead of 4 x 11 + 25 */
	if (!tb && (ts == 2 || two_pass) && !getenv("AT_ROWS_PER_LANE") && ((l1 + 1023) / 1024) * (16 * 11 + 25) < ((l1 + 255) / 256) * (4 * 11 + 25)) L.k = 16;
	/* overlap (one state: few registers even with pointers): 4 or 16 rows per lane, whichever needs fewer instructions */
	if (overlap) L.k = env_ll("AT_ROWS_PER_LANE", 0) == 4 ? 4 : ((l1 + 1023) / 1024) * (16 * 9 + 45) < ((l1 + 255) / 256) * (4 * 9 + 30) ? 16 : 4;
	if (force_g == 64) {
		/* the sliver of a batch behind its whole rounds (align_device), ragged overlap: one group of 64 lanes, whatever the read length */
		if (force_k) L.k = force_k;
	} else if (force_g == 32) {
		/* ragged frames of reads of 305 .. 608 bases, or (force_k) the sliver behind a batch of narrow-group items: one strip on two
		 * groups of 32 lanes */
		L.g = 32;
		L.k = force_k ? force_k : at::class_rows(at::kClass32, l1, at::kClass32RagFirst);
	} else if (!force_g && (g_forced == 0 || g_forced == 4) && ts == 4 && l1 <= at::class_top(at::kClass4)) {
		/* reads of up to 76 bases: sixteen groups of 4 lanes x 9 / 10 / 13 / 16 / 19 rows, 32 alignments per wave */
		L.g = 4;
		L.k = at::class_rows(at::kClass4, l1);
	} else if (force_g != 16 && (force_g == 8 || g_forced == 0 || g_forced == 8) && ts == 4 && l1 <= at::class_top(at::kClass8)) {
		L.g = 8;
		L.k = at::class_rows(at::kClass8, l1);
	} else if ((force_g == 16 || g_forced != 64) && ts == 4 && l1 <= 208) {
		L.g = 16;
		L.k = at::class_rows(at::kClass16, l1);
	} else if ((force_g == 16 || (!force_g && g_forced != 64 && g_forced != 32)) && ts == 4 && l1 > 208 && l1 <= at::class_top(at::kClass16)) {
		/* 250- and 300-base reads: still four groups of 16 lanes, 16 or 19 rows per lane (8 alignments per wave; AT_GROUP=32: the
		 * two 32-lane groups below) */
		L.g = 16;
		L.k = at::class_rows(at::kClass16, l1);
	} else if (g_forced != 64 && ts == 4 && l1 > 208 &&
	           l1 <= (force_g || g_forced == 32 ? at::kTopFit : kmode == at::K_LOCAL ? at::kTopLocal : kmode == at::K_GLOBAL ? at::kTopGlobal : at::kTopFit)) {
		/* 250- and 300-base reads: two groups of 32 lanes (4 alignments per wave); one group of 64 lanes would carry 2 and
		 * cut 300 rows into a strip of 256 and one of 44 */
		L.g = 32;
		/* 305 .. 608 bases: still one strip -- 10, 12, 13, 16 or 19 rows per lane (AT_GROUP=32: the round-1 classes only, 417+ on the
		 * 64-lane groups).  16 rows only for local and global, 19 only for local: the others spill there (268 .. 612 bytes of
		 * scratch per lane) and lose to the strips of the 64-lane group (global 560 / 608 bases: -4 %) */
		L.k = at::class_rows(at::kClass32, l1, 0, g_forced == 32 ? at::kClass32SkipUnderGroup32 : 0);
	}
	const int ng = 64 / L.g;
	const int blk = L.g <= 16 ? 4 : 8;        /* BLK of at_sweep16 */
	const int tbk = (l2 + L.g - 1 + blk - 1) / blk;
	L.ptr_lanes = L.g == 64 ? std::max(1, std::min(64, (l1 + L.k - 1) / L.k)) : 64;
	L.ptr_lanes = (L.ptr_lanes + 3) & ~3;     /* the HBM slot stores 16 bytes per lane: keep every group of rows aligned */
	const long long nstrips = (l1 + L.g * L.k - 1) / (L.g * L.k);
	long long nref = (at::kPad + (long long)tbk * blk) / 4 + 4;
	nref = (nref + 1) & ~1LL;
	/* (two-pass tracebacks: the boundary row's words double as the replay's staging area and the walkers' tile cache) */
	/* (... the replay's rows above, CK + 1 entries of two words per lane; then every walker's copy of the block it walks) */
	const long long walk_words = ((L.k + 3) / 4 + (hasj ? ((L.k + 3) / 4 + 3) / 4 : 0)) * (long long)at::ck_steps(L.g);
	const long long nbound = std::max<long long>(2LL * (l2 + 2), two_pass == 1 ? std::max<long long>(at::ck_stage_words(at::ck_steps(L.g)), 2 * ng * walk_words * (L.g == 64 ? 4 : 1)) : 0);
	/* steps per pointer word (and alignment): 4-bit cells, 4; the jump state with scores x4 keeps byte cells, 2 -- with scores x16 it has
	 * 4-bit cells plus a bit plane of one word per 4 rows x 4 steps behind the cells (at_sweep16.hip.h: JPL); packed overlap: 2-bit cells, 8 */
	const int spw = overlap ? 16 / AT_OVL_BITS : (hasj && !(ts == 4 && AT_JPLANE)) ? 2 : 4;
	const long long njpl = tb && hasj && ts == 4 && AT_JPLANE ? nstrips * tbk * (blk / 4) * ((L.k + 3) / 4) * L.ptr_lanes : 0;
	const long long nptr = tb ? nstrips * tbk * (blk / spw) * L.k * L.ptr_lanes + njpl + 64 : 0;
	const long long nsm = hasj ? (((long long)l2 + 64 + 64 + 128 + 31) / 32 + 2 + 1) & ~1LL : 0;
	L.off_refb = (int)nref;
	L.off_bound = (int)(2 * nref * ng);
	L.off_sm = (int)(2 * nref * ng + nbound);
	L.nsm = (int)nsm;
	L.off_ptr = (int)((2 * nref * ng + nbound + nsm + 3) & ~3LL);   /* 16-byte aligned: wide pointer stores */
	L.words = L.off_ptr + nptr;
	return L;
}

/* Scores of every real (non -inf) cell lie in [-lo, hi]; the packed kernel needs
 * 16*(lo + hi) plus slack below 2^15 so that the -32768 sentinel, even after the
 * hi*16 it can gain along a diagonal of matches, stays below every real value. */
static bool packed_ok(const at_handle *h, int mode, int bits, int l1, int l2, int ts, int *thresh16)
{
	const long long scale = 1LL << ts;
	if (getenv("AT_NO_PACKED") && atoi(getenv("AT_NO_PACKED"))) return false;
	if ((bits != 2 && bits != 8) || l1 < 1 || l2 < 1) return false;   /* 2-bit codes: score LUT; bytes: compare */
	if (mode == AT_MODE_OVERLAP) {
		/* one state, linear gap (alignment.h:926-964; -e unused): scores x4 with 2-bit tags only.  A cell's value is at least
		 * that of the path along its row from column 0 (where M = 0): -|o| * j; at most m * min(l1, l2) */
		if (ts != 2 || h->m < 0 || h->u > 0 || h->o > 0) return false;
		const long long lo = std::llabs((long long)h->o) * std::max(l1, l2) + std::llabs((long long)h->u) + 16;
		const long long hi = (long long)h->m * std::min(l1, l2), slack = std::llabs((long long)h->o) + std::llabs((long long)h->u) + 3;
		if (scale * (lo + hi + slack) >= 32768) return false;
		*thresh16 = (int)(-32768 + scale * (hi + slack));
		return true;
	}
	if (!(mode == AT_MODE_GLOBAL || mode == AT_MODE_LOCAL || mode == AT_MODE_FIT)) return false;
	if (h->m < 0 || h->u > 0 || h->o > 0 || h->e > 0) return false;
	const bool hasj = mode == AT_MODE_FIT && h->use_jump;
	if (hasj && (h->j > 0 || std::llabs((long long)h->j - h->o) * scale > 32000)) return false;
	const long long A = std::max<long long>(std::max(std::llabs((long long)h->e), std::llabs((long long)h->u)), h->m);
	/* global / fit: a cell's value is a max over paths, hence at least the value of one of them -- min(i, j) diagonal
	 * steps, each >= u, and one gap of |i - j|, >= o + e * |i - j|; the L and U states lie at most one more opening below */
	(void)A;
	long long lo = 3 * std::llabs((long long)h->o) + (hasj ? std::llabs((long long)h->j) : 0) +
	               std::llabs((long long)h->u) * std::min(l1, l2) + std::llabs((long long)h->e) * std::max(l1, l2) + 16;
	/* local: M >= 0 everywhere (the 0 candidate, alignment.h:826), so L and U, each the max of something and M + o, never
	 * drop below o, and no cell or intermediate below o + u + e: the matrix has no -inf and no downward drift */
	if (mode == AT_MODE_LOCAL) lo = std::llabs((long long)h->o) + std::llabs((long long)h->u) + std::llabs((long long)h->e) + 16;
	const long long hi = (long long)h->m * std::min(l1, l2);
	const long long slack = std::llabs((long long)h->o) + std::llabs((long long)h->e) + 3;
	if (scale * (lo + hi + slack) >= 32768) return false;
	*thresh16 = (int)(-32768 + scale * (hi + slack));
	return true;
}

/* Two-pass tracebacks (at_sweep16.hip.h, CK kernels): the regions of a wave's global slot -- border row, row checkpoints, column
 * checkpoints, the replayed blocks' pointer words and jump plane -- for the scores-only layout L of the sweep */
struct TpLayout {
	int off_brow, off_rck, off_cck, off_rptr, off_rjpl;
	long long words;
	long long brow_words;
};
/* split: pass 2 is a kernel of its own -- the regions of a work item (row and column checkpoints); the border row is the launch's */
static TpLayout tp_layout(const Layout16 &L, int kmode, int l2, bool split = false)
{
	const int blk = L.g <= 16 ? 4 : 8, cb = at::ck_steps(L.g);
	const long long T = (long long)((l2 + L.g - 1 + blk - 1) / blk) * blk;   /* steps of a sweep */
	const int es = 2, nq = ((kmode == at::K_FITJ ? 3 : 2) * L.k + 3) / 4, kg = (L.k + 3) / 4;
	auto up4 = [](long long v) { return (v + 3) & ~3LL; };
	TpLayout t;
	long long w = 0;
	t.brow_words = (T + cb + 2) * es;
	t.off_brow = (int)w; if (!split) w = up4(w + (T + cb + 2) * es);
	t.off_rck = (int)w; w = up4(w + 64 * es + (T / cb + 3) * 64 * cb * es);   /* (ck_rck_word: the border entries, then tiles of steps) */
	t.off_cck = (int)w; w = up4(w + (T / cb + 3) * ((nq + AT_CK_COL_QUAD - 1) / AT_CK_COL_QUAD * AT_CK_COL_QUAD) * 256);   /* (ck_cck_word: chunks in groups of AT_CK_COL_QUAD) */
	t.off_rptr = (int)w; if (!split) w = up4(w + (cb / 4) * ((L.k + 3) / 4) * 256);   /* [4 steps][4 rows][lane][row in group] */
	t.off_rjpl = (int)w; if (!split) w = up4(w + (cb / 4) * ((kg + 3) / 4) * 256);
	t.words = split ? (w + 63) & ~63LL : w;
	return t;
}

static int choose_store(long long words_fixed, long long words_ptr, bool prefer_hbm_pointers);
/* is there a packed instantiation for the storage class plan_launch will choose for this layout? */
static bool packed16_kernel_exists(int kmode, const Layout16 &P, bool tb, int ts, int bits, int rag, const Layout16 *PT = nullptr)
{
	/* (the launch plans with the larger of the main items' layout and the sliver items': the same maximum here) */
	const long long fixed = PT ? std::max(P.off_ptr, PT->off_ptr) : P.off_ptr;
	const long long ptrw = PT ? std::max(P.words - P.off_ptr, PT->words - PT->off_ptr) : P.words - P.off_ptr;
	const int st = choose_store(fixed, ptrw, P.g < 64 || rag);   /* (ragged frames exist with the pointers in the global slots only) */
	if (P.g != 64 && st == 2) return false;
	return (rag ? at_pick16_rag(kmode, P.g, P.k, st, tb, bits) : at_pick16(kmode, P.g, P.k, ts, st, tb, bits)) != nullptr;
}

/* AT_DIAG_FAIL_ALLOC=ck / ws: that buffer's next hipMalloc asks for 2^50 bytes, so the runtime itself refuses (tests of the fallbacks
 * and of the error state a failed allocation leaves; no device memory is held) */
static bool diag_fail_alloc(const char *which)
{
	const char *v = getenv("AT_DIAG_FAIL_ALLOC");
	return which && v && strcmp(v, which) == 0;
}

static int grow(at_handle *h, void **p, size_t *have, size_t need, const char *which = nullptr)
{
	if (need <= *have) return AT_OK;
	if (*p) { (void)hipFree(*p); *p = nullptr; *have = 0; }
	need = need + need / 8 + 4096;
	if (diag_fail_alloc(which)) need = (size_t)1 << 50;
	hipError_t e = hipMalloc(p, need);
	if (e != hipSuccess) {
		*p = nullptr;
		(void)hipGetLastError();   /* the runtime keeps the failure as the thread's last error: the next launch check (ours or the caller's) would report it */
		return fail(h, AT_ERR_NOMEM, "hipMalloc(%zu): %s", need, hipGetErrorString(e));
	}
	*have = need;
	return AT_OK;
}

/* grow() for the handle's buffers of words (d_ws, d_ck) */
static int grow_words(at_handle *h, uint32_t **p, size_t *have, size_t need, const char *which)
{
	void *v = *p;
	const int rc = grow(h, &v, have, need, which);
	*p = (uint32_t *)v;
	return rc;
}

/* page-locked host memory, grow-only */
static int grow_pinned(at_handle *h, void **p, size_t *have, size_t need)
{
	if (need <= *have) return AT_OK;
	if (*p) { (void)hipHostFree(*p); *p = nullptr; *have = 0; }
	need = need + need / 4 + 4096;
	hipError_t e = hipHostMalloc(p, need, hipHostMallocDefault);
	if (e != hipSuccess) {
		*p = nullptr;
		(void)hipGetLastError();   /* (as in grow) */
		return fail(h, AT_ERR_NOMEM, "hipHostMalloc(%zu): %s", need, hipGetErrorString(e));
	}
	*have = need;
	return AT_OK;
}

/* The mask goes up from page-locked memory with an event behind the copy, so the host waits for nothing: a caller who changes the
 * scoring between two launches queued on one stream keeps both queued.  (It used to go up from a temporary, with a wait for the
 * whole stream behind the copy: every fit -s launch after at_set_scoring stalled the host until the launches before it had
 * drained.)  A staging buffer is written again only once its event has passed; with AT_SITE_STAGES uploads pending the host waits
 * for the oldest.  The device copy is ordered like any other use of the handle's buffers: by the stream. */
enum { AT_SITE_STAGES = 8 };
static int ensure_sitemask(at_handle *h, int max_l2, hipStream_t stream)
{
	if (!h->sitemask_dirty && h->sitemask_for_l2 >= max_l2) return AT_OK;
	const size_t nbits = (size_t)max_l2 + 64 + 64 + 128;
	const size_t nw = (nbits + 31) / 32 + 2;
	at_handle::SiteStage *st = nullptr;
	for (at_handle::SiteStage &c : h->site_stage)
		if (hipEventQuery(c.done) == hipSuccess) { st = &c; break; }
	(void)hipGetLastError();   /* ("not ready" is an answer, not a failure for the launch check to find) */
	if (!st && h->site_stage.size() < AT_SITE_STAGES) {
		at_handle::SiteStage c;
		HIP_TRY(h, hipEventCreateWithFlags(&c.done, hipEventDisableTiming));
		h->site_stage.push_back(c);
		st = &h->site_stage.back();
	}
	if (!st) {
		st = &h->site_stage[h->site_next++ % AT_SITE_STAGES];
		HIP_TRY(h, hipEventSynchronize(st->done));
	}
	int rc = grow_pinned(h, &st->host, &st->bytes, nw * 4);
	if (rc) return rc;
	uint32_t *m = (uint32_t *)st->host;
	for (size_t w = 0; w < nw; ++w) m[w] = 0xffffffffu;
	/* column j (1-based) may open the jump state iff (j-1) is NOT a listed site
	 * -- the reference's inverted test, alignment.h:659 / SURVEY.md 0.4 */
	for (int sidx : h->sites) {
		const long long j = (long long)sidx + 1;
		if (j < 0 || (size_t)(j + 64) >= nbits) continue;
		m[(size_t)(j + 64) >> 5] &= ~(1u << ((j + 64) & 31));
	}
	void *p = h->d_sitemask; size_t have = h->sitemask_words * 4;
	rc = grow(h, &p, &have, nw * 4);
	h->d_sitemask = (uint32_t *)p; h->sitemask_words = have / 4;
	if (rc) return rc;
	HIP_TRY(h, hipMemcpyAsync(h->d_sitemask, m, nw * 4, hipMemcpyHostToDevice, stream));
	HIP_TRY(h, hipEventRecord(st->done, stream));
	h->sitemask_dirty = false;
	h->sitemask_for_l2 = max_l2;
	return AT_OK;
}

/* the handle's work counter block (128 bytes, zeroed when it is made); every launch starts with its work counter at zero */
static int ensure_queue(at_handle *h, hipStream_t stream)
{
	if (!h->d_queue) { HIP_TRY(h, hipMalloc((void **)&h->d_queue, 128)); HIP_TRY(h, hipMemset(h->d_queue, 0, 128)); }
	HIP_TRY(h, hipMemsetAsync(h->d_queue, 0, 8, stream));
	return AT_OK;
}

/* Storage class + grid for one launch.
 *   store 0  s2 window, boundary row and pointer matrix in LDS
 *   store 1  s2 + boundary in LDS, pointer matrix in a per-wave global slot (HBM/L2)
 *   store 2  everything in the global slot (very long s2)
 * Work is handed out through an atomic counter, so the grid only has to cover the waves that
 * can be resident; over-estimating it is harmless. */
struct Plan {
	int store, off_ptr;
	long long grid, slot_words;
	size_t dyn_lds;
	uint32_t *ws;
};

/* storage class for (fixed, pointer) words per work item; no side effects (also used to ask whether a kernel exists) */
static int choose_store(long long words_fixed, long long words_ptr, bool prefer_hbm_pointers)
{
	/* all-LDS only while at least 8 waves (2 per SIMD) still fit a CU: measured, occupancy beyond 1 wave/SIMD is
	 * worth +30..50 % on this issue-bound kernel (profiles/r01) */
	const long long limit_all = env_ll("AT_SMALL_LDS_LIMIT", 20 * 1024);
	const long long limit_fixed = env_ll("AT_MEDIUM_LDS_LIMIT", 64 * 1024);
	const long long forced = env_ll("AT_STORE", -1);
	int store;
	if (forced >= 0 && forced <= 2) store = (int)forced;
	else if ((words_fixed + words_ptr) * 4 <= limit_all) store = 0;
	else if (words_fixed * 4 <= limit_fixed) store = 1;
	else store = 2;
	/* several alignments per wave (16- and 32-lane groups): the pointer matrices in LDS would cap the CU at a few waves
	 * even when they fit (49-base reads: 1 151 GCUPS all-LDS, 1 357 with the slots in HBM) */
	if (prefer_hbm_pointers && forced < 0 && store == 0 && words_ptr > 0) store = 1;
	if (words_ptr == 0 && store == 1) store = 0;
	if (store < 2 && words_fixed * 4 > 150 * 1024) store = 2;
	if (store == 0 && (words_fixed + words_ptr) * 4 > 150 * 1024) store = 1;
	return store;
}

static int plan_launch(at_handle *h, const char *tag, int k, long long nwork, long long words_fixed, long long words_ptr,
                       Plan *pl, hipStream_t stream, const std::function<const void *(int)> &kernel_for_store,
                       bool prefer_hbm_pointers = false)
{
	const int store = choose_store(words_fixed, words_ptr, prefer_hbm_pointers);
	const long long lds_words = store == 0 ? words_fixed + words_ptr : (store == 1 ? words_fixed : 0);
	const long long slot_words = store == 0 ? 0 : (((store == 1 ? words_ptr : words_fixed + words_ptr) + 63) & ~63LL);
	long long per_cu = 16;
	if (lds_words > 0) per_cu = std::min<long long>(per_cu, (long long)(h->lds_per_cu - 512) / std::max<long long>(lds_words * 4, 256));
	per_cu = std::max(1LL, std::min(per_cu, env_ll("AT_WAVES_PER_CU", 16)));
	{   /* what the register file really admits */
		int occ = 0;
		const void *fn = kernel_for_store ? kernel_for_store(store) : nullptr;
		if (fn && hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, 64, (size_t)lds_words * 4) == hipSuccess && occ > 0)
			per_cu = std::min<long long>(per_cu, occ);
	}
	long long grid = std::max(1LL, std::min<long long>(nwork, per_cu * h->ncu));
	/* (Tried and dropped: shrinking the grid so that every wave gets the same number of items -- fewer resident
	 * waves cost 5-13 % more than the partial last round they avoid.) */
	pl->store = store;
	pl->off_ptr = store == 1 ? 0 : (int)words_fixed;
	pl->dyn_lds = (size_t)lds_words * 4;
	pl->slot_words = slot_words;
	pl->ws = nullptr;
	if (slot_words > 0) {
		const long long cap = env_ll("AT_WS_CAP_MB", 16384) << 20;
		if (slot_words * 4 > cap) return fail(h, AT_ERR_NOMEM, "one pair needs %lld workspace bytes (cap %lld)", slot_words * 4, cap);
		grid = std::max(1LL, std::min(grid, cap / (slot_words * 4)));
		if (int rc = grow_words(h, &h->d_ws, &h->ws_bytes, (size_t)(grid * slot_words * 4), "ws")) return rc;
		pl->ws = h->d_ws;
	}
	pl->grid = grid;
	if (int rcq = ensure_queue(h, stream)) return rcq;
	static const char *names[3] = {"lds", "lds+hbm-pointers", "hbm"};
	snprintf(h->cfg, sizeof h->cfg, "%s store=%s rows/lane=%d lds=%zuB slot=%lldB waves/cu<=%lld grid=%lld", tag, names[store], k,
	         pl->dyn_lds, slot_words * 4, per_cu, grid);
	return AT_OK;
}

/* One batch launch, as align_device takes it.  Every entry fills one by field name; the per-call settings start as the handle's
 * and an entry that needs others (the scans' window pass, at_allpairs_hits) overrides them HERE: the handle is not written while
 * a call runs (its helper handles run chunks side by side), ck_alloc_failed -- a fact about the handle's lifetime -- excepted */
struct BatchReq {
	int mode = 0;
	int64_t npairs = 0;
	const uint32_t *d_seq = nullptr;
	int bits = 2;
	const int64_t *d_woff1 = nullptr, *d_woff2 = nullptr;
	const int32_t *d_len1 = nullptr, *d_len2 = nullptr;
	int32_t max_len1 = 0, max_len2 = 0;
	int uniform_shape = 0, want_traceback = 0;
	int32_t *d_score = nullptr, *d_end_i = nullptr, *d_end_j = nullptr, *d_state = nullptr;
	uint8_t *d_ops = nullptr;
	const int64_t *d_ops_off = nullptr;
	int32_t *d_nops = nullptr;
	hipStream_t stream = nullptr;
	int64_t ap_n = 0, ap_first = 0;           /* all-vs-all: pair p of the launch is pair ap_first + p of the triangle over ap_n reads */
	const int *d_order = nullptr;             /* the processing order of a ragged batch */
	int rag = 0;                              /* ragged frames: their group width (the host entry) */
	const int *only_if = nullptr;             /* the launch is a no-op unless *only_if == only_val (auto-uniform) */
	int only_val = 0;
	/* ---- per-call settings ---- */
	int edit_infix = 0, edit_tb = 0;          /* at_set_edit_infix, at_set_edit_traceback */
	int infix_anchor = 0;                     /* at_scan_hits' window pass: infix alignments end in (l1, l2) (InfixArgs::anchor_end) */
	int min_on = 0, min_score = 0;            /* at_set_min_score */
	const char *no_walk = nullptr;            /* no walk kernel for this call: the reason, as at_last_config says it */

	explicit BatchReq(const at_handle *h)
	{
		if (h) { edit_infix = h->edit_infix; edit_tb = h->edit_tb; min_on = h->min_on; min_score = h->min_score; }
	}
};

static int align_device(at_handle *h, const BatchReq &r);

extern "C" int at_align_batch_device(at_handle *h, int mode, int64_t npairs,
                                     const uint32_t *d_seq, int bits,
                                     const int64_t *d_woff1, const int32_t *d_len1,
                                     const int64_t *d_woff2, const int32_t *d_len2,
                                     int32_t max_len1, int32_t max_len2, int uniform_shape, int want_traceback,
                                     int32_t *d_score, int32_t *d_end_i, int32_t *d_end_j, int32_t *d_state,
                                     uint8_t *d_ops, const int64_t *d_ops_off, int32_t *d_nops, void *stream_)
{
	if (!d_woff2 || !d_len2) return fail(h, AT_ERR_ARG, "NULL device pointer");
	BatchReq r(h);
	r.mode = mode; r.npairs = npairs; r.d_seq = d_seq; r.bits = bits; r.stream = (hipStream_t)stream_;
	r.d_woff1 = d_woff1; r.d_len1 = d_len1; r.d_woff2 = d_woff2; r.d_len2 = d_len2; r.max_len1 = max_len1; r.max_len2 = max_len2;
	r.uniform_shape = uniform_shape; r.want_traceback = want_traceback;
	r.d_score = d_score; r.d_end_i = d_end_i; r.d_end_j = d_end_j; r.d_state = d_state;
	r.d_ops = d_ops; r.d_ops_off = d_ops_off; r.d_nops = d_nops;
	return align_device(h, r);
}

extern "C" int at_align_allpairs_device(at_handle *h, int mode, int64_t nreads,
                                        const uint32_t *d_seq, int bits,
                                        const int64_t *d_woff, const int32_t *d_len, int32_t max_len,
                                        int64_t first_pair, int64_t npairs, int want_traceback,
                                        int32_t *d_score, int32_t *d_end_i, int32_t *d_end_j, int32_t *d_state,
                                        uint8_t *d_ops, const int64_t *d_ops_off, int32_t *d_nops, void *stream_)
{
	if (!h) return fail(nullptr, AT_ERR_ARG, "at_align_allpairs_device: NULL handle");
	if (nreads < 2 || first_pair < 0 || npairs < 0 || first_pair + npairs > nreads * (nreads - 1) / 2)
		return fail(h, AT_ERR_ARG, "all-vs-all: pair range [%lld, +%lld) outside the %lld*(%lld-1)/2 ordered pairs",
		            (long long)first_pair, (long long)npairs, (long long)nreads, (long long)nreads);
	BatchReq r(h);
	r.mode = mode; r.npairs = npairs; r.d_seq = d_seq; r.bits = bits; r.stream = (hipStream_t)stream_;
	r.d_woff1 = r.d_woff2 = d_woff; r.d_len1 = r.d_len2 = d_len; r.max_len1 = r.max_len2 = max_len;
	r.want_traceback = want_traceback;
	r.d_score = d_score; r.d_end_i = d_end_i; r.d_end_j = d_end_j; r.d_state = d_state;
	r.d_ops = d_ops; r.d_ops_off = d_ops_off; r.d_nops = d_nops;
	r.ap_n = nreads; r.ap_first = first_pair;
	return align_device(h, r);
}

extern "C" int at_render_batch_device(at_handle *h, int64_t npairs,
                                      const uint32_t *d_seq, int bits,
                                      const int64_t *d_woff1, const int64_t *d_woff2,
                                      const int32_t *d_end_i, const int32_t *d_end_j,
                                      const uint8_t *d_ops, const int64_t *d_ops_off, const int32_t *d_nops,
                                      uint8_t *d_r1, uint8_t *d_r2, const int64_t *d_str_off, int nul_terminate,
                                      void *stream_)
{
	if (!h) return fail(nullptr, AT_ERR_ARG, "at_render_batch_device: NULL handle");
	if (npairs < 0) return fail(h, AT_ERR_ARG, "negative npairs");
	if (npairs == 0) return AT_OK;
	if (bits != 2 && bits != 8) return fail(h, AT_ERR_ARG, "bits must be 2 or 8");
	if (!d_seq || !d_woff1 || !d_woff2 || !d_end_i || !d_end_j || !d_ops || !d_ops_off || !d_nops || !d_r1 || !d_r2)
		return fail(h, AT_ERR_ARG, "NULL device pointer");
	HIP_TRY(h, hipSetDevice(h->device));
	drop_stale_error();
	hipStream_t s = (hipStream_t)stream_;
	at::RenderArgs ra;
	ra.npairs = npairs; ra.seq = d_seq; ra.woff1 = (const long long *)d_woff1; ra.woff2 = (const long long *)d_woff2;
	ra.end_i = d_end_i; ra.end_j = d_end_j; ra.ops = d_ops; ra.ops_off = (const long long *)d_ops_off; ra.nops = d_nops;
	ra.r1 = d_r1; ra.r2 = d_r2; ra.str_off = (const long long *)d_str_off; ra.nul = nul_terminate ? 1 : 0; ra.bad = h->d_rflag;
	/* four pairs per wavefront, 16 lanes each (AT_RENDER_GROUP = 8 / 32 / 64: A/B runs; 64 = one pair per wavefront, the round-1 form) */
	/* alignments of long pairs are hundreds of ops long: one pair per wavefront again (C3: 2 833 against 2 871 GCUPS with four) */
	const long long rw = env_ll("AT_RENDER_GROUP", h->last_span >= 1024 ? 64 : 16);
	const int w = rw == 64 ? 64 : rw == 32 ? 32 : rw == 8 ? 8 : 16;
	const int per_block = 4 * (64 / w);
	h->last_render_lanes = w;
	const unsigned grid = (unsigned)std::min<int64_t>((npairs + per_block - 1) / per_block, 16LL * h->ncu);
#define AT_RENDER(B, W) hipLaunchKernelGGL((at::at_render_k<B, W>), dim3(grid), dim3(256), 0, s, ra)
	if (bits == 2) { if (w == 64) AT_RENDER(2, 64); else if (w == 32) AT_RENDER(2, 32); else if (w == 8) AT_RENDER(2, 8); else AT_RENDER(2, 16); }
	else { if (w == 64) AT_RENDER(8, 64); else if (w == 32) AT_RENDER(8, 32); else if (w == 8) AT_RENDER(8, 8); else AT_RENDER(8, 16); }
#undef AT_RENDER
	HIP_TRY(h, hipGetLastError());
	return AT_OK;
}

/* exclusive prefix sums of max(nops, 0) into d_off[0 .. npairs] (d_off[npairs] = total) */
static int scan_nops_device(at_handle *h, int64_t npairs, const int32_t *d_nops, int64_t *d_off, hipStream_t s)
{
	const unsigned ntiles = (unsigned)((npairs + at::SCAN_TILE - 1) / at::SCAN_TILE);
	int rc = grow(h, &h->d_scan, &h->scan_bytes, (size_t)ntiles * 8);
	if (rc) return rc;
	hipLaunchKernelGGL(at::at_scan_tiles, dim3(ntiles), dim3(256), 0, s, d_nops, (long long)npairs, (long long *)h->d_scan);
	hipLaunchKernelGGL(at::at_scan_nops, dim3(ntiles), dim3(256), 0, s, d_nops, (long long)npairs, (const long long *)h->d_scan,
	                   (long long *)d_off);
	HIP_TRY(h, hipGetLastError());
	return AT_OK;
}

extern "C" int at_compact_ops_device(at_handle *h, int64_t npairs,
                                     const uint8_t *d_ops, const int64_t *d_ops_off, const int32_t *d_nops,
                                     uint8_t *d_packed, int64_t packed_cap, int64_t *d_packed_off, void *stream_)
{
	if (!h) return fail(nullptr, AT_ERR_ARG, "at_compact_ops_device: NULL handle");
	if (npairs < 0 || packed_cap < 0) return fail(h, AT_ERR_ARG, "negative size");
	if (!d_ops || !d_ops_off || !d_nops || !d_packed || !d_packed_off) return fail(h, AT_ERR_ARG, "NULL device pointer");
	HIP_TRY(h, hipSetDevice(h->device));
	drop_stale_error();
	hipStream_t s = (hipStream_t)stream_;
	if (npairs == 0) {
		HIP_TRY(h, hipMemsetAsync(d_packed_off, 0, 8, s));
		return AT_OK;
	}
	int rc = scan_nops_device(h, npairs, d_nops, d_packed_off, s);
	if (rc) return rc;
	{
		const unsigned grid = (unsigned)std::min<int64_t>((npairs + 15) / 16, 16LL * h->ncu);
		hipLaunchKernelGGL(at::at_compact_k, dim3(grid), dim3(256), 0, s, (long long)npairs, d_ops, (const long long *)d_ops_off,
		                   d_nops, d_packed, (const long long *)d_packed_off, (long long)packed_cap);
	}
	HIP_TRY(h, hipGetLastError());
	return AT_OK;
}

extern "C" int at_cigar_batch_device(at_handle *h, int64_t npairs,
                                     const uint32_t *d_seq, int bits,
                                     const int64_t *d_woff1, const int64_t *d_woff2,
                                     const int32_t *d_end_i, const int32_t *d_end_j,
                                     const uint8_t *d_ops, const int64_t *d_ops_off, const int32_t *d_nops,
                                     int flags, int32_t *d_ncigar, int32_t *d_stats, int64_t *d_cigar_off,
                                     uint32_t *d_cigar, int64_t cigar_cap, void *stream_)
{
	if (!h) return fail(nullptr, AT_ERR_ARG, "at_cigar_batch_device: NULL handle");
	if (npairs < 0 || cigar_cap < 0) return fail(h, AT_ERR_ARG, "negative size");
	if (!d_cigar_off) return fail(h, AT_ERR_ARG, "NULL device pointer");
	HIP_TRY(h, hipSetDevice(h->device));
	drop_stale_error();
	hipStream_t s = (hipStream_t)stream_;
	if (npairs == 0) {
		HIP_TRY(h, hipMemsetAsync(d_cigar_off, 0, 8, s));
		return AT_OK;
	}
	if (bits != 2 && bits != 8) return fail(h, AT_ERR_ARG, "bits must be 2 or 8");
	if (!d_seq || !d_woff1 || !d_woff2 || !d_end_i || !d_end_j || !d_ops || !d_ops_off || !d_nops || !d_ncigar || (!d_cigar && cigar_cap > 0))
		return fail(h, AT_ERR_ARG, "NULL device pointer");
	at::CigarArgs ca;
	ca.npairs = npairs; ca.seq = d_seq; ca.woff1 = (const long long *)d_woff1; ca.woff2 = (const long long *)d_woff2;
	ca.end_i = d_end_i; ca.end_j = d_end_j; ca.ops = d_ops; ca.ops_off = (const long long *)d_ops_off; ca.nops = d_nops;
	ca.merge = (flags & AT_CIGAR_M) ? 1 : 0; ca.ncigar = d_ncigar; ca.stats = d_stats; ca.cigar_off = (const long long *)d_cigar_off;
	ca.cigar = d_cigar; ca.cap = cigar_cap;
	/* the group width of at_render_batch_device, by its rule and its knob (two widths are built: AT_RENDER_GROUP = 64 is one pair per
	 * wavefront, every other value the 16-lane groups) */
	const int w = env_ll("AT_RENDER_GROUP", h->last_span >= 1024 ? 64 : 16) == 64 ? 64 : 16;
	h->last_cigar_lanes = w;
	HIP_TRY(h, at_cigar_launch(&ca, bits, w, 0, h->ncu, s));
	int rc = scan_nops_device(h, npairs, d_ncigar, d_cigar_off, s);
	if (rc) return rc;
	HIP_TRY(h, at_cigar_launch(&ca, bits, w, 1, h->ncu, s));
	return AT_OK;
}

/* ================ the batch dispatch: align_device, at the end, is the routing order; every kernel family has its
 * launcher above it.  A launcher reads the request, never the handle's per-call settings ================ */

/* what the register file admits per CU; the runtime's refusal to say is no reason to fail */
static int occupancy_or_8(const void *fn, size_t lds)
{
	int occ = 0;
	if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, 64, lds) != hipSuccess || occ <= 0) occ = 8;
	return occ;
}

/* what every bit-parallel kernel takes from a request (the queue follows ensure_queue) */
static at::MyersArgs myers_args(const BatchReq &r)
{
	at::MyersArgs m;
	memset(&m, 0, sizeof m);
	m.npairs = r.npairs; m.seq = r.d_seq;
	m.woff1 = (const long long *)r.d_woff1; m.woff2 = (const long long *)r.d_woff2; m.len1 = r.d_len1; m.len2 = r.d_len2;
	m.max_l1 = r.max_len1; m.max_l2 = r.max_len2;
	m.score = r.d_score; m.end_i = r.d_end_i; m.end_j = r.d_end_j; m.state = r.d_state; m.nops = r.d_nops;
	m.order = r.d_order;
	m.ap_n = r.ap_n; m.ap_first = r.ap_first;
	return m;
}

/* The slab of the two op-list edit paths (at_edit_tb, at_infix): one column is W words x 2 planes x 64 lanes per work item, bounded
 * like the pointer slots of plan_launch.  slab_size refuses a work item over the cap (`what` opens the text); slab_grid sizes the
 * grid by the occupancy and the cap and grows d_ws */
struct SlabPlan { long long slab_words = 0, cap = 0, per_cu = 0, grid = 0; };
static int slab_size(at_handle *h, const char *what, const BatchReq &r, int w, SlabPlan *sp)
{
	sp->slab_words = (long long)std::max(r.max_len2, 1) * w * 128;
	sp->cap = env_ll("AT_WS_CAP_MB", 16384) << 20;
	if (sp->slab_words * 4 > sp->cap)
		return fail(h, AT_ERR_NOMEM, "%s: one work item needs %lld workspace bytes (cap %lld)", what, sp->slab_words * 4, sp->cap);
	return AT_OK;
}
static int slab_grid(at_handle *h, const BatchReq &r, int occ, SlabPlan *sp)
{
	sp->per_cu = std::max(1LL, std::min<long long>(occ, env_ll("AT_WAVES_PER_CU", 16)));
	sp->grid = std::max(1LL, std::min<long long>(std::min<long long>((r.npairs + 63) / 64, sp->per_cu * h->ncu), sp->cap / (sp->slab_words * 4)));
	return grow_words(h, &h->d_ws, &h->ws_bytes, (size_t)(sp->grid * sp->slab_words * 4), "ws");
}

/* ---- edit infix mode (at_set_edit_infix): the best match of s1 inside s2 on the bit-parallel path with a zero top border
 * (at_infix.hip.h), with the op lists when edit alignments are on and wanted.  Outside the domain the call fails: a global
 * distance under an infix setting would be a wrong answer ---- */
static int launch_infix(at_handle *h, const BatchReq &r)
{
	const bool itb = r.want_traceback && r.edit_tb;
	const size_t lds = at::myers_window_bytes(64, r.max_len2);   /* the 64 s2 windows of a wavefront */
	if (r.ap_n > 0) return fail(h, AT_ERR_DOMAIN, "edit infix mode: no all-vs-all (pair lists and searches only)");
	if (h->u != 1) return fail(h, AT_ERR_DOMAIN, "edit infix mode needs the unit mismatch cost: u = %d, not 1", h->u);
	if (r.bits != 2) return fail(h, AT_ERR_DOMAIN, "edit infix mode needs a 2-bit batch: some base is not one of ACGT");
	if (r.max_len1 > 1024) return fail(h, AT_ERR_DOMAIN, "edit infix mode: max_len1 = %d exceeds 1024", r.max_len1);
	if (lds > 60 * 1024) return fail(h, AT_ERR_DOMAIN, "edit infix mode: max_len2 = %d exceeds 3792 (64 windows of packed words in 60 KB of LDS)", r.max_len2);
	if (r.rag || r.only_if) return fail(h, AT_ERR_ARG, "edit infix mode: not a packed launch");
	const int w = at::class_rows(at::kMyersLaneWords, r.max_len1);
	at_infix_fn fn = at_pick_infix(w, itb ? 1 : 0);
	if (!fn) return fail(h, AT_ERR_ARG, "no edit infix kernel for %d words per lane", w);
	const int occ = occupancy_or_8((const void *)fn, lds);
	at::InfixArgs ia;
	memset(&ia, 0, sizeof ia);
	ia.m = myers_args(r);
	SlabPlan sp;
	if (itb) {
		/* the slab of at_edit_tb, the same caps (the op buffers are there: align_device has looked) */
		int rc = slab_size(h, "edit infix alignments", r, w, &sp);
		if (!rc) rc = slab_grid(h, r, occ, &sp);
		if (rc) return rc;
		ia.ops = r.d_ops; ia.ops_off = (const long long *)r.d_ops_off;
		ia.slab = h->d_ws; ia.slab_words = sp.slab_words;
		ia.anchor_end = r.infix_anchor;
	} else {
		/* sized as the number-only launch of at_myers, one alignment per lane */
		sp.grid = std::max(1LL, std::min<long long>((r.npairs + 63) / 64, (long long)occ * h->ncu));
	}
	if (int rcq = ensure_queue(h, r.stream)) return rcq;
	ia.m.queue = h->d_queue;
	hipLaunchKernelGGL(fn, dim3((unsigned)sp.grid), dim3(64), lds, r.stream, ia);
	HIP_TRY(h, hipGetLastError());
	if (itb)
		snprintf(h->cfg, sizeof h->cfg, "myers-infix-tb bits=2 words/lane=%d (64 pairs/wave) lds=%zuB slab=%lldB waves/cu<=%lld grid=%lld", w, lds,
		         sp.slab_words * 4, sp.per_cu, sp.grid);
	else
		snprintf(h->cfg, sizeof h->cfg, "myers-infix bits=2 words/lane=%d (64 pairs/wave) lds=%zuB waves/cu<=%d grid=%lld", w, lds, occ, sp.grid);
	return AT_OK;
}

/* ---- edit alignments (at_set_edit_traceback): the bit-parallel fill keeps its columns, the same wavefront walks them
 * (at_edit_tb.hip.h).  Outside the domain the call fails: no silent fall back to the number alone ---- */
static int launch_edit_tb(at_handle *h, const BatchReq &r)
{
	const size_t lds = at::myers_window_bytes(64, r.max_len2);   /* the 64 s2 windows of a wavefront */
	if (h->u != 1) return fail(h, AT_ERR_DOMAIN, "edit alignments need the unit mismatch cost: u = %d, not 1", h->u);
	if (r.bits != 2) return fail(h, AT_ERR_DOMAIN, "edit alignments need a 2-bit batch: some base is not one of ACGT");
	if (r.max_len1 > 1024) return fail(h, AT_ERR_DOMAIN, "edit alignments: max_len1 = %d exceeds 1024", r.max_len1);
	if (lds > 60 * 1024) return fail(h, AT_ERR_DOMAIN, "edit alignments: max_len2 = %d exceeds 3792 (64 windows of packed words in 60 KB of LDS)", r.max_len2);
	const int w = at::class_rows(at::kMyersLaneWords, r.max_len1);
	at_edit_tb_fn fn = at_pick_edit_tb(w);
	if (!fn) return fail(h, AT_ERR_ARG, "no edit alignment kernel for %d words per lane", w);
	SlabPlan sp;
	int rc = slab_size(h, "edit alignments", r, w, &sp);
	if (!rc) rc = slab_grid(h, r, occupancy_or_8((const void *)fn, lds), &sp);
	if (rc) return rc;
	at::EditTbArgs ea;
	memset(&ea, 0, sizeof ea);
	ea.m = myers_args(r);
	ea.ops = r.d_ops; ea.ops_off = (const long long *)r.d_ops_off;
	ea.slab = h->d_ws; ea.slab_words = sp.slab_words;
	if (int rcq = ensure_queue(h, r.stream)) return rcq;
	ea.m.queue = h->d_queue;
	hipLaunchKernelGGL(fn, dim3((unsigned)sp.grid), dim3(64), lds, r.stream, ea);
	HIP_TRY(h, hipGetLastError());
	snprintf(h->cfg, sizeof h->cfg, "myers-tb bits=2 words/lane=%d (64 pairs/wave) lds=%zuB slab=%lldB waves/cu<=%lld grid=%lld", w, lds,
	         sp.slab_words * 4, sp.per_cu, sp.grid);
	return AT_OK;
}

/* ---- edit distance with unit mismatch cost: bit-parallel kernel (at_myers.hip.h), any mix of lengths ---- */
/* (two s2 windows of a wavefront must fit 60 KB of LDS, or the cell-by-cell kernel takes the batch) */
static bool myers_takes(const at_handle *h, const BatchReq &r, int kmode)
{
	return kmode == at::K_EDIT && h->u == 1 && r.bits == 2 && r.max_len1 <= 32768 && at::myers_window_bytes(2, r.max_len2) <= 60 * 1024 &&
	       env_ll("AT_MYERS", 1);
}

static int launch_myers(at_handle *h, const BatchReq &r)
{
	/* (bytes of LDS for the s2 windows of the n alignments of a wavefront) */
	auto myers_windows = [&](int n) { return at::myers_window_bytes(n, r.max_len2); };
	/* lanes per alignment and words per lane: reads of up to AT_MYERS_LANE_MAX (1 024) bases one alignment per LANE -- 5, 8, 16 or 32
	 * words, 64 s2 windows in LDS (second sequences of up to ~3 500 bases) -- else 32 lanes; the 16- and 32-word forms only for batches
	 * of AT_MYERS_LANE_MIN_PAIRS (16 384: one wavefront per CU) and more -- 10 000 pairs of 1 000 x 1 000 are 157 wavefronts on 1 024
	 * SIMDs, 19 TCUPS against 31 on 32-lane groups; 131 072 of them 43 against 36.  AT_MYERS_GROUP = 8: the round-2 form, eight lanes
	 * for reads of up to 256 bases and 32 beyond (A/B) */
	const long long lane_max = env_ll("AT_MYERS_LANE_MAX", 1024);
	const bool per_lane = r.max_len1 <= lane_max && r.max_len1 <= 1024 && myers_windows(64) <= 60 * 1024 &&
	                      (r.max_len1 <= 256 || r.npairs >= env_ll("AT_MYERS_LANE_MIN_PAIRS", 16384)) && env_ll("AT_MYERS_GROUP", 1) == 1;
	const int g = per_lane ? 1 : r.max_len1 <= 256 && myers_windows(8) <= 60 * 1024 ? 8 : 32;
	const int w = per_lane ? at::class_rows(at::kMyersLaneWords, r.max_len1) : at::class_rows(at::kMyersGroupWords, r.max_len1);
	at_myers_fn fn = at_pick_myers(w, g);
	const int per_wave = 64 / g;
	at::MyersArgs m = myers_args(r);
	if (int rcq = ensure_queue(h, r.stream)) return rcq;
	m.queue = h->d_queue;
	const size_t lds = myers_windows(per_wave);
	if (lds > 60 * 1024) return fail(h, AT_ERR_RANGE, "second sequence too long for the bit-parallel kernel's LDS window");
	const int occ = occupancy_or_8((const void *)fn, lds);
	const long long grid = std::max(1LL, std::min<long long>((r.npairs + per_wave - 1) / per_wave, (long long)occ * h->ncu));
	hipLaunchKernelGGL(fn, dim3((unsigned)grid), dim3(64), lds, r.stream, m);
	HIP_TRY(h, hipGetLastError());
	snprintf(h->cfg, sizeof h->cfg, "myers bits=2 words/lane=%d %dx%d-lane groups (%d pairs/wave) lds=%zuB waves/cu<=%d grid=%lld", w, per_wave, g, per_wave,
	         lds, occ, grid);
	return AT_OK;
}

/* ---- all-vs-all overlap scores with a threshold (at_set_min_score): the bit-parallel filter (at_myers.hip.h, SEMI) bounds every
 * pair's score from above at a seventh of the sweep's cost; only pairs whose bound reaches the threshold are swept.  The filter
 * leaves (upper bound, state 0) in every pair's result slot and the candidates' indices in a list; the int32 sweep takes the
 * list and its length from the device and overwrites the candidates' slots with exact results.  No host round trip.
 * Where the filter applies, *cand_order and *cand_count are that list and its length on the device and `note` opens the
 * sweep's at_last_config; elsewhere all three stay as they are ---- */
static int overlap_filter(at_handle *h, const BatchReq &r, int kmode, bool tb, const int **cand_order, const int **cand_count, char (&note)[96])
{
	if (!(kmode == at::K_OVERLAP && !tb && r.ap_n > 0 && r.min_on && !r.d_order && !r.only_if && r.bits == 2 && r.max_len1 >= 1 && r.max_len1 <= 1024 &&
	      r.npairs < (1LL << 31) - 64 && env_ll("AT_OVERLAP_FILTER", 1)))
		return AT_OK;
	/* 2 score <= 2 m b - (2 c - m) D', c = min(m - u, m / 2 - o): needs m >= 0 and 2 c > m */
	const long long k2 = std::min<long long>(2LL * (h->m - h->u), (long long)h->m - 2LL * h->o) - h->m;
	const int w = at::class_rows(at::kMyersLaneWords, r.max_len1);
	at_myers_fn ffn = at_pick_myers_semi(w);
	const size_t lds = at::myers_window_bytes(64, r.max_len2);
	if (!(h->m >= 0 && k2 > 0 && k2 < 4096 && h->m < 4096 && lds <= 60 * 1024 && ffn)) return AT_OK;
	int rc = grow(h, &h->d_order, &h->order_bytes, ((size_t)r.npairs + 64) * 4);
	if (rc) return rc;
	int *cand = (int *)h->d_order, *count = cand + ((r.npairs + 15) & ~15LL);
	HIP_TRY(h, hipMemsetAsync(count, 0, 4, r.stream));
	at::MyersArgs m = myers_args(r);
	m.nops = nullptr;   /* (scores only: the bound has no op counts) */
	m.semi_m2 = 2 * h->m; m.semi_k = (int)k2; m.semi_min2 = (int)std::max<long long>(std::min<long long>(2LL * r.min_score, INT32_MAX), INT32_MIN);
	m.cand_order = cand; m.cand_count = count;
	if (int rcq = ensure_queue(h, r.stream)) return rcq;
	m.queue = h->d_queue;
	const int occ = occupancy_or_8((const void *)ffn, lds);
	const long long fgrid = std::max(1LL, std::min<long long>((r.npairs + 63) / 64, (long long)occ * h->ncu));
	hipLaunchKernelGGL(ffn, dim3((unsigned)fgrid), dim3(64), lds, r.stream, m);
	HIP_TRY(h, hipGetLastError());
	*cand_order = cand; *cand_count = count;
	snprintf(note, sizeof note, "overlap filter (bit-parallel bound, %d words/lane, min score %d) + ", w, r.min_score);
	return AT_OK;
}

/* ---- the int32 sweep: every mode, any mix of lengths.  d_order: the request's, or the overlap filter's candidates with their
 * count in *npairs_dev and the filter's note ---- */
static int launch_int32(at_handle *h, const BatchReq &r, int kmode, bool tb, const int *d_order, const int *npairs_dev, const char *filter_note)
{
	/* the int32 kernels read 2-bit scores from a byte LUT (the packed ones from a 16-bit one) */
	if (r.bits == 2 && !scores_fit_byte(h, r.mode))
		return fail(h, AT_ERR_RANGE, "the int32 2-bit kernels need |16*score| <= 127 (m=%d u=%d o=%d): pack the batch with bits=8", h->m, h->u, h->o);
	const Layout L = layout_for(kmode, r.bits, tb, r.max_len1, r.max_len2);
	if (L.words >= (1LL << 30)) return fail(h, AT_ERR_RANGE, "pair too large: %lld workspace words", L.words);
	SweepArgs a;
	memset(&a, 0, sizeof a);
	a.npairs = r.npairs;
	a.seq = r.d_seq;
	a.woff1 = (const long long *)r.d_woff1; a.len1 = r.d_len1;
	a.woff2 = (const long long *)r.d_woff2; a.len2 = r.d_len2;
	a.m16 = h->m * 16; a.u16 = h->u * 16; a.o16 = h->o * 16; a.e16 = h->e * 16; a.g16 = h->j * 16;
	a.u_raw = h->u;
	a.score = r.d_score; a.end_i = r.d_end_i; a.end_j = r.d_end_j; a.state = r.d_state;
	a.ops = r.d_ops; a.ops_off = (const long long *)r.d_ops_off; a.nops = r.d_nops;
	a.off_bound = L.off_bound; a.ptr_lanes = L.ptr_lanes; a.off_sm = L.off_sm; a.nsm = L.nsm;
	a.ap_n = r.ap_n; a.ap_first = r.ap_first; a.order = d_order;
	a.only_if = r.only_if; a.only_val = r.only_val;
	a.npairs_dev = npairs_dev;
	if (kmode == at::K_FITJ) {
		int rc = ensure_sitemask(h, r.max_len2, r.stream);
		if (rc) return rc;
		a.sitemask = h->d_sitemask;
	}
	Plan pl;
	char tag[32];
	snprintf(tag, sizeof tag, "int32 bits=%d", r.bits);
	int rc = plan_launch(h, tag, L.k, r.npairs, L.off_ptr, L.words - L.off_ptr, &pl, r.stream, [&](int st) {
		return (const void *)(r.bits == 2 ? at_pick32_b2(kmode, L.k, st, tb) : at_pick32_b8(kmode, L.k, st, tb));
	});
	if (rc) return rc;
	a.off_ptr = pl.off_ptr; a.ws = pl.ws; a.ws_slot_words = pl.slot_words; a.queue = h->d_queue;
	a.max_l1 = r.max_len1; a.max_l2 = r.max_len2;
	at_sweep_fn fn = r.bits == 2 ? at_pick32_b2(kmode, L.k, pl.store, tb) : at_pick32_b8(kmode, L.k, pl.store, tb);
	if (pl.dyn_lds > 48 * 1024)
		HIP_TRY(h, hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.dyn_lds));
	hipLaunchKernelGGL(fn, dim3((unsigned)pl.grid), dim3(64), pl.dyn_lds, r.stream, a);
	HIP_TRY(h, hipGetLastError());
	if (filter_note[0]) {
		const std::string tail = h->cfg;
		snprintf(h->cfg, sizeof h->cfg, "%s%.200s", filter_note, tail.c_str());
	}
	return AT_OK;
}

/* ---- auto-uniform: the caller did not promise one shape, but the batch may well have one (fixed-length reads against fixed
 * windows).  The lengths live on the device and this entry is asynchronous, so the device decides: a check kernel leaves 1 in a
 * flag if every pair is max_len1 x max_len2, and the packed and the int32 launch are both queued, each of them a no-op unless the
 * flag names it ---- */
static bool auto_uniform_applies(const at_handle *h, const BatchReq &r, int kmode)
{
	int thresh16 = 0;
	return !r.uniform_shape && !r.rag && !r.only_if && r.ap_n == 0 && r.npairs >= 4096 && !r.d_order && kmode <= at::K_FITJ &&
	       env_ll("AT_AUTO_UNIFORM", 1) && (r.bits == 8 || scores_fit_byte(h, r.mode)) &&
	       packed_ok(h, r.mode, r.bits, r.max_len1, r.max_len2, 4, &thresh16);
}

static int launch_auto_uniform(at_handle *h, const BatchReq &r)
{
	int *flag = h->d_rflag + 8;
	HIP_TRY(h, hipMemsetAsync(flag, 0xff, 4, r.stream));
	const unsigned cg = (unsigned)std::min<int64_t>((r.npairs + 255) / 256, 4LL * h->ncu);
	hipLaunchKernelGGL(at::at_check_uniform, dim3(cg), dim3(256), 0, r.stream, r.d_len1, r.d_len2, (long long)r.npairs, r.max_len1, r.max_len2, flag);
	BatchReq guarded_req = r;
	guarded_req.only_if = flag;
	guarded_req.uniform_shape = 1; guarded_req.only_val = -1;
	int rc = align_device(h, guarded_req);
	if (rc) return rc;
	const std::string packed_cfg = h->cfg;
	guarded_req.uniform_shape = 0; guarded_req.only_val = 0;
	rc = align_device(h, guarded_req);
	if (rc) return rc;
	snprintf(h->cfg, sizeof h->cfg, "auto: [%.140s] if every pair is %dx%d, else [%.120s]", packed_cfg.c_str(), r.max_len1, r.max_len2,
	         std::string(h->cfg).c_str());
	return AT_OK;
}

/* ---- packed int16 path: uniform shape (or ragged frames), scores provably within 16 bits ---- */
/* what route_packed decides: ts = 0 -- not this path */
struct Packed16 {
	int ts = 0;            /* scores x16 with nibble pointers when they fit (|score| < 2048), else x4 with byte pointers (|score| < 8192) */
	int thresh16 = 0;
	Layout16 P;
	bool two_pass = false;
	int tp_split = 0;      /* pass 2: 0 the rounds inside the sweep's kernel, 1 a walk kernel behind it */
	const char *ck_note = "";
};

static int route_packed(at_handle *h, const BatchReq &r, int kmode, bool tb, Packed16 *pk)
{
	const int32_t max_len1 = r.max_len1, max_len2 = r.max_len2;
	const int rag = r.rag, bits = r.bits;
	int ts = 0;
	if ((r.uniform_shape || rag) && r.ap_n == 0) {
		if (packed_ok(h, r.mode, bits, max_len1, max_len2, 4, &pk->thresh16)) ts = 4;
		else if ((!rag || kmode == at::K_OVERLAP) && packed_ok(h, r.mode, bits, max_len1, max_len2, 2, &pk->thresh16)) ts = 2;
		/* overlap: the packed kernel exists with pointers only (scores alone: the int32 kernel's 2 instructions per cell win) */
		if (kmode == at::K_OVERLAP && (!tb || getenv("AT_NO_PACKED_OVERLAP"))) ts = 0;
	}
	if (rag && (!ts || (kmode > at::K_FITJ && !(kmode == at::K_OVERLAP && rag == 64)) || max_len1 > at::rag_group_top(rag) || !r.d_order))
		return fail(h, AT_ERR_ARG, "ragged packed launch outside its domain");   /* the host entry checks before it asks */
	Layout16 &P = pk->P;
	if (ts) {
		P = layout16_for(tb, kmode == at::K_FITJ, max_len1, max_len2, ts, rag, kmode == at::K_OVERLAP, kmode,
		                 rag && kmode == at::K_OVERLAP ? at::class_rows(at::kClassOvl, max_len1) : 0);   /* (ragged overlap: one strip) */
		/* A 64-lane packed wave carries 2 alignments where an int32 wave carries 1: fewer, longer work items.  A batch
		 * that cannot give every resident wave one of them stays on the int32 kernel.  (10k x 1024^2 = 1.6 rounds: 1.96
		 * packed vs 2.00 TCUPS int32 for a lone launch, 2.70 vs 2.13 with launches in flight; 61k pairs: 2.70 vs 2.19.)  Not a ragged launch:
		 * its order is padded with ~index repeats, which only the packed kernels understand */
		const double min_rounds = getenv("AT_PACKED_MIN_ROUNDS") ? atof(getenv("AT_PACKED_MIN_ROUNDS")) : 1.0;
		if (!rag && P.g == 64 && (double)((r.npairs + 1) / 2) < min_rounds * 12.0 * h->ncu) ts = 0;
		/* the packed kernels index their slot with 24-bit multiplies: a pair whose slot would not fit takes the int32 kernel */
		if (P.words >= (1LL << 24)) { if (rag) return fail(h, AT_ERR_ARG, "ragged packed launch outside its domain (slot too large)"); ts = 0; }
		/* no packed kernel for the storage class this shape needs (the 16- and 32-lane groups have no all-HBM variant:
		 * a 150-base read against a second sequence of more than ~4 000 bases): the int32 kernel takes any length */
		Layout16 PTq = P;
		const bool tailq = !rag && !r.only_if && P.g <= 16 && kmode != at::K_OVERLAP && env_ll("AT_TAIL_SPLIT", 1);
		if (tailq) PTq = layout16_for(tb, kmode == at::K_FITJ, max_len1, max_len2, ts, at::AT_TAIL_G, false, kmode, at::at_tail_k(P.g, P.k));
		if (ts && !packed16_kernel_exists(kmode, P, tb, ts, bits, rag, tailq ? &PTq : nullptr)) {
			if (rag) return fail(h, AT_ERR_ARG, "ragged packed launch outside its domain (frame too long for LDS)");
			ts = 0;
		}
	}
	/* two-pass tracebacks: uniform batches whose shape has a CK kernel sweep without pointers and rebuild them where the walks go.
	 * By default where that wins -- the 64-lane groups with 16 rows per lane (reads of 609 .. 1 024 bases: the one-pass kernels hold 4 rows
	 * per lane there and need four strips); AT_TWO_PASS=2: wherever a CK kernel exists (the 8-lane groups x 19 rows lose: C2 -7 %, C4
	 * -28 %, profiles/r04/two_pass_ab.txt), AT_TWO_PASS=0: never (A/B runs) */
	const long long tp_mode = env_ll("AT_TWO_PASS", 1);
	if (ts && tb && !rag && kmode <= at::K_FITJ && tp_mode) {
		Layout16 P2 = layout16_for(false, kmode == at::K_FITJ, max_len1, max_len2, ts, 0, false, kmode, 0, 1);
		/* pass 2 as a kernel of its own (at_walk16.hip.h): the sweep leaves its checkpoints per work item, walkers replay the blocks their
		 * walks cross.  By default on the 64-lane groups, where teams of walker lanes cut the chain of rounds (C3 2 940 -> 4 420 GCUPS with
		 * launches in flight, 2 150 -> 3 310 one at a time, against the one-pass kernels), and on the 8-lane groups for fit against a long
		 * second sequence (tp_split_narrow_default); AT_TP_SPLIT=1: wherever a walk kernel exists, 0: nowhere (the rounds inside the sweep's kernel) */
		const bool narrow_default = P2.g == 8 && tp_split_narrow_default(kmode, max_len1, max_len2);
		const bool split_default = P2.g == 64 || narrow_default;
		const bool split_want = env_ll("AT_TP_SPLIT", split_default ? 1 : 0) && at_pick_walk16(kmode, P2.g, P2.k, ts, bits);
		const int split_req = split_want && !h->ck_alloc_failed && !r.no_walk ? 1 : 0;
		/* (the fallback without a checkpoint buffer: the rounds inside the sweep's kernel on the 64-lane groups, the one-pass kernels on the
		 * 8-lane groups -- at_last_config says so) */
		if (split_want && !split_req) pk->ck_note = r.no_walk ? r.no_walk : " [checkpoint buffer unavailable on this handle: no separate pass 2]";
		if ((P2.g == 64 || tp_mode >= 2 || (split_req && narrow_default)) && (long long)P2.g * P2.k >= max_len1 && at_pick16_tp(kmode, P2.g, P2.k, ts, bits) &&
		    choose_store(P2.off_ptr, 1, true) == 1) {
			pk->two_pass = true;
			pk->tp_split = split_req;
			if (pk->tp_split) P2 = layout16_for(false, kmode == at::K_FITJ, max_len1, max_len2, ts, 0, false, kmode, 0, 2);
			P = P2;
		}
	}
	pk->ts = ts;
	return AT_OK;
}

/* a walker lane's pointer words of one block, and the walk kernel's LDS (at_walk16.hip.h, walk16_lds_words) */
static long long walk_lane_words(int kmode, const Layout16 &L)
{
	const int cb = at::ck_steps(L.g);
	return L.k * (cb / 4) + (kmode == at::K_FITJ ? (L.k + 3) / 4 * (cb / 4) : 0);
}
static size_t walk_lds(int kmode, const Layout16 &L, bool ptr_in_lds)
{
	const int cb = at::ck_steps(L.g), nsm = kmode == at::K_FITJ ? L.nsm : 0;
	return (size_t)((nsm + 1) / 2 * 2 + (L.k > 16 ? 0 : (cb + 1) * 128) + (ptr_in_lds ? 64 * walk_lane_words(kmode, L) : 0)) * 4;
}

/* pass 2 of a piece as a kernel of its own, behind the piece's sweep: b the main items, bt the sliver's; *wnote: the walkers note, also
 * appended to at_last_config */
static int launch_walk16(at_handle *h, const BatchReq &r, int kmode, const Packed16 &pk, const Layout16 &PT, bool tail_ok,
                         const Sweep16Args &b, const Sweep16Args &bt, std::string *wnote)
{
	const Layout16 &P = pk.P;
	const int64_t nm = b.npairs, n_tail = bt.npairs;
	/* the 64-lane groups: teams of lanes per pair of alignments (walk16_team_wave; AT_WALK_TEAMS=0: one walker per half-lane there too) */
	const bool teams = env_ll("AT_WALK_TEAMS", P.g == 64 ? 1 : 0) && at_pick_walk16(kmode, P.g, P.k, pk.ts, r.bits, 1);
	at_walk16_fn wf = at_pick_walk16(kmode, P.g, P.k, pk.ts, r.bits, teams);
	if (!wf) return fail(h, AT_ERR_RANGE, "no walk kernel for %d-lane groups x %d rows", P.g, P.k);
	const size_t lds = std::max(walk_lds(kmode, P, true), tail_ok ? walk_lds(kmode, PT, true) : 0);
	if (lds > 48 * 1024) HIP_TRY(h, hipFuncSetAttribute((const void *)wf, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
	/* the main units' walkers: one wavefront per 128 alignments (LDS admits four per CU; the others queue).  AT_WALK_WAVES_PER_CU = n:
	 * at most n per CU, persistent, which refill their halves from the counters behind the sweep's work counter -- fewer
	 * wavefront-rounds, but a chain of them per wavefront: C4 one launch at a time 1 450 (n = 1) / 1 820 (2) / 2 160 GCUPS (all),
	 * C2 2 300 / 2 490 / 2 500, with launches in flight 2 270 / 2 370 / 2 390 and 3 130 / 3 130 / 3 140 */
	const long long wcap = env_ll("AT_WALK_WAVES_PER_CU", 0);
	const long long wmain = std::max<long long>(1, wcap > 0 ? std::min<long long>((nm + 127) / 128, wcap * h->ncu) : (nm + 127) / 128);
	HIP_TRY(h, hipMemsetAsync(h->d_queue + 8, 0, 16, r.stream));
	const int tpw = 64 / at_walk16_team_lanes(P.g);   /* teams per wavefront */
	const long long wteams = ((nm + 1) / 2 + tpw - 1) / tpw;
	hipLaunchKernelGGL(wf, dim3((unsigned)((teams ? wteams : wmain) + (n_tail + 127) / 128)), dim3(64), lds, r.stream, b, bt);
	/* (the main alignments' walker wavefronts: with fewer than one per 128 alignments, they refill from the counters) */
	char note[128];
	snprintf(note, sizeof note, " [walkers: %lld wavefronts%s for %lld alignments]", teams ? wteams : wmain, teams ? " of teams" : "", (long long)nm);
	cfg_append(h, "%s", note);
	*wnote = note;
	HIP_TRY(h, hipGetLastError());
	return AT_OK;
}

/* The sliver of a piece: the last n_tail pairs of b leave it and come back as the items of the sliver's layout PT (npairs = 0: no
 * sliver) */
static Sweep16Args split_sliver(Sweep16Args &b, int64_t n_tail, const Layout16 &PT)
{
	Sweep16Args bt = b;
	bt.npairs = 0;
	if (n_tail <= 0) return bt;
	const int64_t nm = b.npairs - n_tail;
	b.npairs = nm;
	bt.npairs = n_tail;
	bt.woff1 += nm; bt.woff2 += nm; bt.len1 += nm; bt.len2 += nm;
	bt.score += nm;
	if (bt.end_i) bt.end_i += nm;
	if (bt.end_j) bt.end_j += nm;
	if (bt.state) bt.state += nm;
	if (bt.ops_off) bt.ops_off += nm;
	if (bt.nops) bt.nops += nm;
	bt.off_refb = PT.off_refb; bt.off_bound = PT.off_bound; bt.ptr_lanes = PT.ptr_lanes; bt.off_sm = PT.off_sm; bt.nsm = PT.nsm;
	return bt;
}

static int launch_packed(at_handle *h, const BatchReq &r, int kmode, bool tb, const Packed16 &pk)
{
	const Layout16 &P = pk.P;
	const int ts = pk.ts, tp_split = pk.tp_split, rag = r.rag, bits = r.bits;
	const bool two_pass = pk.two_pass;
	const int32_t max_len1 = r.max_len1, max_len2 = r.max_len2;
	const int64_t npairs = r.npairs;
	const int per_wave = 2 * (64 / P.g);
	/* the sliver's layout (see below) */
	const bool tail_ok = !rag && !r.only_if && P.g <= 16 && kmode != at::K_OVERLAP && env_ll("AT_TAIL_SPLIT", 1) &&
	                     (!tp_split || P.g == 8);   /* (the walk kernels of the 8-lane groups carry their sliver's walks) */
	Layout16 PT = P;
	if (tail_ok) PT = layout16_for(tb && !two_pass, kmode == at::K_FITJ, max_len1, max_len2, ts, at::AT_TAIL_G, false, kmode, at::at_tail_k(P.g, P.k), two_pass ? (tp_split ? 2 : 1) : 0);
	TpLayout tpm{}, tpt{};
	if (two_pass) { tpm = tp_layout(P, kmode, max_len2, tp_split != 0); tpt = tp_layout(PT, kmode, max_len2, tp_split != 0); }
	/* split two-pass: the checkpoints of a whole launch live side by side -- C2 225 KB, C3 / C4 1.1 MB per work item -- so a batch is
	 * swept and walked in pieces whose checkpoints fit AT_CK_CAP_MB (8 192) */
	int64_t piece = npairs;
	int64_t brow_words = 0;
	if (tp_split) {
		const long long cap = env_ll("AT_CK_CAP_MB", 8192) << 20;
		brow_words = (tpm.brow_words + 63) & ~63LL;
		const long long tail_reserve = tail_ok ? 16LL * h->ncu * tpt.words * 4 : 0;
		const long long items = (cap - tail_reserve - brow_words * 4) / (tpm.words * 4 + 16LL * per_wave);
		if (items < 1) {
			/* not even one work item's checkpoints fit the cap: this batch without the walk kernel (nothing has been launched yet) */
			BatchReq again = r;
			again.no_walk = " [one work item's checkpoints exceed AT_CK_CAP_MB: no separate pass 2]";
			return align_device(h, again);
		}
		piece = std::min<int64_t>(npairs, items * per_wave);
		const long long forced = env_ll("AT_CK_PIECE_PAIRS", 0);   /* (tests: pieces of this many pairs, whatever the cap) */
		if (forced > 0) piece = std::min<int64_t>(piece, std::max<long long>(1, forced / per_wave) * per_wave);
	}
	std::string cfg_first, walk_last;   /* (at_last_config: the first piece's configuration, the last piece's walkers) */
	for (int64_t first = 0; first < npairs; first += piece) {
		const int64_t np = std::min<int64_t>(piece, npairs - first);
		Sweep16Args b;
		memset(&b, 0, sizeof b);
		b.npairs = np; b.seq = r.d_seq;
		b.woff1 = (const long long *)r.d_woff1 + first; b.woff2 = (const long long *)r.d_woff2 + first;
		b.len1 = r.d_len1 + first; b.len2 = r.d_len2 + first;
		b.l1 = max_len1; b.l2 = max_len2;
		const int sc = 1 << ts;
		b.m16 = h->m * sc; b.u16 = h->u * sc; b.o16 = h->o * sc; b.e16 = h->e * sc; b.g16 = h->j * sc; b.thresh16 = pk.thresh16;
		if (kmode == at::K_FITJ) {
			int rcs = ensure_sitemask(h, max_len2, r.stream);
			if (rcs) return rcs;
			b.sitemask = h->d_sitemask;
		}
		b.score = r.d_score + first; b.end_i = r.d_end_i ? r.d_end_i + first : nullptr; b.end_j = r.d_end_j ? r.d_end_j + first : nullptr;
		b.state = r.d_state ? r.d_state + first : nullptr;
		b.ops = r.d_ops; b.ops_off = r.d_ops_off ? (const long long *)r.d_ops_off + first : nullptr; b.nops = r.d_nops ? r.d_nops + first : nullptr;
		b.order = rag ? r.d_order : nullptr;
		b.only_if = r.only_if; b.only_val = r.only_val;
		b.off_refb = P.off_refb; b.off_bound = P.off_bound; b.ptr_lanes = P.ptr_lanes; b.off_sm = P.off_sm; b.nsm = P.nsm;
		Plan pl;
		char tag16[192];
		snprintf(tag16, sizeof tag16, "packed16 x%d bits=%d %dx%d-lane groups (%d pairs/wave)%s", 1 << ts, bits, 64 / P.g, P.g, per_wave,
		         rag ? " ragged frames" : "");
		if (two_pass) snprintf(tag16 + strlen(tag16), sizeof tag16 - strlen(tag16), " two-pass%s ck=%d", tp_split ? " (walk kernel)" : "", at::ck_steps(P.g));
		/* local 2-bit batches with scores x16 whose scoring allows it (m >= 0 >= u, (m - u) * 16 in a byte) run the kernels with the
		 * profile lookup (at_sweep16.hip.h, PROF): the same results, 0.84 of an instruction per row-step less.  Every other scoring
		 * keeps the kernels with the score LUT.  With tracebacks in one pass those kernels also take the cell maximum with one three-input
		 * float maximum on biased scores, which holds the batch's frame to max3_domain_ok (m * min(l1, l2) <= 944 and |o| + |u| + |e| <= 959):
		 * a batch outside it keeps the LUT kernels too */
		const bool prof = kmode == at::K_LOCAL && bits == 2 && ts == 4 && at::profile_lookup_ok(h->m, h->u) &&
		                  (!(tb && !two_pass) || at::max3_domain_ok(h->m, h->u, h->o, h->e, max_len1, max_len2));
		/* (which form ran, for at_last_config and tools/route_dump.py) */
		if (kmode == at::K_LOCAL && ts == 4)
			snprintf(tag16 + strlen(tag16), sizeof tag16 - strlen(tag16), "%s", !prof ? " [score LUT]" : tb && !two_pass ? " [profile words, biased max3]" : " [profile words]");
		auto pick = [&](int st) {
			if (two_pass) return st == 1 ? at_pick16_tp(kmode, P.g, P.k, ts, bits, tp_split, prof) : (at_sweep16_fn) nullptr;
			return rag ? at_pick16_rag(kmode, P.g, P.k, st, tb, bits, prof) : at_pick16(kmode, P.g, P.k, ts, st, tb, bits, prof);
		};
		const long long nwork = (np + per_wave - 1) / per_wave;
		/* The grid is the resident waves, each pulling work items until none are left.  A SIMD holds two of these waves and finishes
		 * an item every ~118 us: C2's 6 250 items of 16 pairs on 1 024 SIMDs are 6.1 items per SIMD, so a launch that has the chip to
		 * itself ends with 106 SIMDs working through a 7th item while the others idle (0.86 ms instead of 0.72).  When such a sliver
		 * remains (the last round less than a quarter full), its pairs become items of two 32-lane groups -- four alignments per wave,
		 * items a third as long -- that follow the main items IN THE SAME LAUNCH and work queue (the kernel's second argument,
		 * at_sweep16.hip.h).  AT_TAIL_SPLIT=0: off.  (Round 2 ran the sliver as a second launch behind the
		 * main one, which cost a caller who keeps launches in flight 8 %; round 3 first tried it on a stream of its own beside the
		 * main launch: +6.5 % alone, -8 % in flight -- the next batch's waves took the slots the sliver was waiting for.) */
		/* (the sliver's items use the main items' LDS window and pointer slot: both hold either layout -- the main items' are the larger) */
		int rc = plan_launch(h, tag16, P.k, nwork, std::max(P.off_ptr, PT.off_ptr),
		                     tp_split ? 64 : two_pass ? std::max(tpm.words, tpt.words) : std::max(P.words - P.off_ptr, PT.words - PT.off_ptr), &pl, r.stream,
		                     [&](int st) { return (const void *)pick(st); }, P.g < 64 || rag || two_pass);
		if (rc) return rc;
		if (tp_split) {
			/* AT_TP_RESERVE=n: the sweep leaves n wave slots per CU to the walk kernels of the launches around it (its waves are
			 * persistent: a walk kernel queued behind it otherwise waits for the whole sweep of the NEXT launch to drain) */
			const long long rsv = env_ll("AT_TP_RESERVE", 0) * h->ncu;
			if (rsv > 0 && pl.grid > rsv && nwork > pl.grid - rsv) {
				pl.grid = std::max<long long>(h->ncu, pl.grid - rsv);
				cfg_append(h, " (AT_TP_RESERVE: sweep grid=%lld)", pl.grid);
			}
		}
		int64_t n_tail = 0;
		if (tail_ok && nwork > pl.grid) {
			const long long sliver = nwork % pl.grid;
			if (sliver > 0 && sliver * 4 <= pl.grid) n_tail = np - (nwork - sliver) * per_wave;   /* (four 32-lane items per 8-lane item: one per SIMD at most) */
		}
		Sweep16Args bt = split_sliver(b, n_tail, PT);
		const int64_t nm = np - n_tail;
		b.off_ptr = pl.off_ptr; b.ws = pl.ws; b.ws_slot_words = pl.slot_words; b.queue = h->d_queue;
		bt.off_ptr = pl.store == 1 ? 0 : PT.off_ptr; bt.ws = pl.ws; bt.ws_slot_words = pl.slot_words; bt.queue = h->d_queue;
		if (two_pass) {
			if (pl.store != 1) return fail(h, AT_ERR_RANGE, "two-pass tracebacks need the s2 windows in LDS (store=%d)", pl.store);
			b.off_brow = tpm.off_brow; b.off_rck = tpm.off_rck; b.off_cck = tpm.off_cck; b.off_rptr = tpm.off_rptr; b.off_rjpl = tpm.off_rjpl;
			bt.off_brow = tpt.off_brow; bt.off_rck = tpt.off_rck; bt.off_cck = tpt.off_cck; bt.off_rptr = tpt.off_rptr; bt.off_rjpl = tpt.off_rjpl;
		}
		if (tp_split) {
			/* [row 0 | end cells of the np alignments | the main items' checkpoints | the sliver items'] */
			const long long n_main_items = (nm + per_wave - 1) / per_wave, n_tail_items = (n_tail + 2 * (64 / at::AT_TAIL_G) - 1) / (2 * (64 / at::AT_TAIL_G));
			const long long end_words = ((np * 4) + 63) & ~63LL;
			const size_t need = (size_t)(brow_words + end_words + n_main_items * tpm.words + n_tail_items * tpt.words) * 4;
			const std::string err_before = h->err, g_err_before = g_err;
			rc = grow_words(h, &h->d_ck, &h->ck_bytes, need, "ck");
			if (rc && first == 0) {
				/* no room for a launch's checkpoints (several handles on one card, a small AT_CK_CAP_MB would have cut the batch into pieces):
				 * nothing has been launched yet -- the same batch with the rounds inside the sweep's kernel, whose checkpoints live in the
				 * resident wavefronts' slots.  A fallback that works is no error: the hipMalloc text goes again */
				h->ck_alloc_failed = true;
				rc = align_device(h, r);
				if (rc == AT_OK) {
					snprintf(h->err, sizeof h->err, "%s", err_before.c_str());
					snprintf(g_err, sizeof g_err, "%s", g_err_before.c_str());
				}
				return rc;
			}
			if (rc) return rc;
			b.ck_brow = h->d_ck; bt.ck_brow = h->d_ck;
			b.tp_end = (int4 *)(h->d_ck + brow_words); bt.tp_end = b.tp_end + nm;
			b.ck = h->d_ck + brow_words + end_words; b.ck_item_words = tpm.words;
			bt.ck = b.ck + n_main_items * tpm.words; bt.ck_item_words = tpt.words;
		}
		at_sweep16_fn fn16 = pick(pl.store);
		if (!fn16 || (P.g != 64 && pl.store == 2)) return fail(h, AT_ERR_RANGE, "no packed kernel for this shape (rows/lane=%d, store=%d)", P.k, pl.store);
		if (pl.dyn_lds > 48 * 1024)
			HIP_TRY(h, hipFuncSetAttribute((const void *)fn16, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.dyn_lds));
		hipLaunchKernelGGL(fn16, dim3((unsigned)pl.grid), dim3(64), pl.dyn_lds, r.stream, b, bt);
		HIP_TRY(h, hipGetLastError());
		/* (diagnostic builds, -DAT_DIAG_SWEEP_ONLY=1: AT_DIAG_NO_WALK_KERNEL=1 -- throw-away runs without pass 2: what does the sweep alone
		 * reach?  Every pair reports garbage ops.  The product ignores the knob) */
		if (tp_split && !(AT_DIAG_SWEEP_ONLY && env_ll("AT_DIAG_NO_WALK_KERNEL", 0))) {
			rc = launch_walk16(h, r, kmode, pk, PT, tail_ok, b, bt, &walk_last);
			if (rc) return rc;
		}
		if (n_tail > 0)
			cfg_append(h, " + last %lld pairs as 32-lane items (rows/lane=%d)", (long long)n_tail, PT.k);
		if (first == 0) cfg_first = h->cfg;
	}
	if (piece < npairs) snprintf(h->cfg, sizeof h->cfg, "%.360s; in pieces of %lld pairs%s%s", cfg_first.c_str(), (long long)piece,
	                              walk_last.empty() ? "" : "; last piece", walk_last.c_str());
	if (pk.ck_note[0]) cfg_append(h, "%s", pk.ck_note);
	return AT_OK;
}

/* The routing order.  A rung that takes the batch returns; the two fallbacks of the packed path come back in here with the same
 * request (the cap fallback with no_walk set, before anything was queued; the allocation fallback with ck_alloc_failed set, after
 * plan_launch and the site mask's upload of the first piece, before any launch) */
static int align_device(at_handle *h, const BatchReq &r)
{
	if (!h) return fail(nullptr, AT_ERR_ARG, "at_align_batch_device: NULL handle");
	if (r.mode < AT_MODE_GLOBAL || r.mode > AT_MODE_EDIT) return fail(h, AT_ERR_ARG, "unknown mode %d", r.mode);
	if (r.npairs < 0 || r.max_len1 < 0 || r.max_len2 < 0) return fail(h, AT_ERR_ARG, "negative size");
	if (r.bits != 2 && r.bits != 8) return fail(h, AT_ERR_ARG, "bits must be 2 or 8");
	if (r.npairs == 0) return AT_OK;
	if (!r.d_seq || !r.d_woff1 || !r.d_len1 || !r.d_woff2 || !r.d_len2 || !r.d_score) return fail(h, AT_ERR_ARG, "NULL device pointer");
	/* edit alignments (at_set_edit_traceback): batches only -- the all-pairs entries keep the number */
	const bool edit_tb = r.want_traceback && r.mode == AT_MODE_EDIT && r.edit_tb && r.ap_n == 0;
	const bool tb = r.want_traceback && r.mode != AT_MODE_EDIT;
	if ((tb || edit_tb) && (!r.d_ops || !r.d_ops_off || !r.d_nops)) return fail(h, AT_ERR_ARG, "traceback wanted but ops buffers are NULL");
	HIP_TRY(h, hipSetDevice(h->device));
	drop_stale_error();

	/* exact-int32 range: real scores stay within 2^24, sentinel at -2^26 (at_sweep.hip.h) */
	long long maxabs = 0;
	for (int v : {h->m, h->u, h->o, h->e, h->j}) maxabs = std::max<long long>(maxabs, std::llabs((long long)v));
	maxabs = std::max<long long>(maxabs, 1);
	if (maxabs * ((long long)r.max_len1 + r.max_len2 + 2) >= (1LL << 24))
		return fail(h, AT_ERR_RANGE, "scores may exceed the exact range: max|param|=%lld, l1+l2=%lld", maxabs,
		            (long long)r.max_len1 + r.max_len2);

	h->last_span = r.max_len1 + r.max_len2;
	const int kmode = r.mode == AT_MODE_GLOBAL ? at::K_GLOBAL : r.mode == AT_MODE_LOCAL ? at::K_LOCAL
	                : r.mode == AT_MODE_FIT ? (h->use_jump ? at::K_FITJ : at::K_FIT)
	                : r.mode == AT_MODE_OVERLAP ? at::K_OVERLAP : at::K_EDIT;

	if (r.mode == AT_MODE_EDIT && r.edit_infix) return launch_infix(h, r);
	if (auto_uniform_applies(h, r, kmode)) return launch_auto_uniform(h, r);
	Packed16 pk;
	if (int rc = route_packed(h, r, kmode, tb, &pk)) return rc;
	if (pk.ts) return launch_packed(h, r, kmode, tb, pk);
	if (edit_tb) return launch_edit_tb(h, r);
	if (myers_takes(h, r, kmode)) return launch_myers(h, r);
	const int *order = r.d_order, *npairs_dev = nullptr;
	char filter_note[96] = "";
	if (int rc = overlap_filter(h, r, kmode, tb, &order, &npairs_dev, filter_note)) return rc;
	return launch_int32(h, r, kmode, tb, order, npairs_dev, filter_note);
}

/* ---- host entry: 2-bit packing while staging (round 4) ----
 * The host entry used to copy every raw byte into page-locked memory and send it up (30 MB per 100k pairs of C2), the GPU packed.
 * The staging pass already touches every byte: it now packs them -- 16 bases per word, the layout of at_pack<2> -- so a quarter of
 * the bytes cross the link, and the sweeps, which wait for their chunk's upload, start that much earlier.  32 bases per step:
 * code = ((c >> 1) ^ (c >> 2)) & 3 maps A C G T to 0 1 2 3, a byte shuffle of "ACGT" by the code must give the byte back (else the
 * batch is not pure ACGT: the raw path takes over, as before), two multiply-adds fold four codes into a byte. */
#if defined(__x86_64__)
#include <immintrin.h>
__attribute__((target("avx2"))) static inline __m256i pack2_step(__m256i v, __m256i bad, uint32_t *dst)
{
	const __m256i m3 = _mm256_set1_epi8(3), w14 = _mm256_set1_epi16(0x0401), w116 = _mm256_set1_epi32(0x00100001);
	const __m256i acgt = _mm256_setr_epi8('A', 'C', 'G', 'T', 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 'A', 'C', 'G', 'T', 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0);
	const __m256i pickb = _mm256_setr_epi8(0, 4, 8, 12, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, 0, 4, 8, 12, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1);
	const __m256i code = _mm256_and_si256(_mm256_xor_si256(_mm256_srli_epi16(v, 1), _mm256_srli_epi16(v, 2)), m3);
	const __m256i x = _mm256_madd_epi16(_mm256_maddubs_epi16(code, w14), w116);   /* a byte per 4 bases in every dword */
	const __m256i y = _mm256_shuffle_epi8(x, pickb);
	const uint64_t r = (uint64_t)(uint32_t)_mm256_extract_epi32(y, 0) | ((uint64_t)(uint32_t)_mm256_extract_epi32(y, 4) << 32);
	memcpy(dst, &r, 8);
	return _mm256_or_si256(bad, _mm256_xor_si256(_mm256_shuffle_epi8(acgt, code), v));
}
/* `len` bytes of ACGT -> (len + 15) / 16 + 1 words (the last one the padding word the kernels' windows read ahead into); false if a
 * byte is not one of ACGT (the words are then unspecified) */
__attribute__((target("avx2"))) static bool pack2_avx2(const uint8_t *src, int len, uint32_t *dst)
{
	const int nw = (len + 15) / 16 + 1;
	__m256i bad = _mm256_setzero_si256();
	int b = 0;
	for (; b + 32 <= len; b += 32) bad = pack2_step(_mm256_loadu_si256((const __m256i *)(src + b)), bad, dst + b / 16);
	if (b < len) {   /* (the last 1 .. 31 bases, filled up with A = code 0: its two words end at or before the padding word) */
		alignas(32) uint8_t tail[32];
		memset(tail, 'A', 32);
		memcpy(tail, src + b, (size_t)(len - b));
		bad = pack2_step(_mm256_load_si256((const __m256i *)tail), bad, dst + b / 16);
	}
	dst[nw - 1] = 0;
	return _mm256_testz_si256(bad, bad) != 0;
}
static bool host_pack_available() { static const bool ok = __builtin_cpu_supports("avx2"); return ok; }
#else
static bool pack2_avx2(const uint8_t *, int, uint32_t *) { return false; }
static bool host_pack_available() { return false; }
#endif

/* AT_HOST_TRACE=1: microseconds since the first call at the stages of the host entry, on stderr (where does a call's time go?) */
static void htrace(const char *what, long long a)
{
	static const bool on = getenv("AT_HOST_TRACE") != nullptr;
	if (!on) return;
	static const auto t0 = std::chrono::steady_clock::now();
	const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
	fprintf(stderr, "[host %10.1f us] %s %lld\n", us, what, a);
}

/* the CIGAR form of the host entry (at_align_batch_cigar): what a chunk fills in.  The words stay in the chunk's own page-locked
 * buffer (at_handle::cg_words, cg_total) until the parent lays the chunks' payloads back to back in pair order (cigar_gather) */
struct CigarReq {
	int flags;
	int32_t *out_stats, *out_ncigar;
	int64_t *out_off;              /* [n] the chunk's own exclusive offsets; the parent adds the words of the chunks before it */
};

/* host-buffer entry; with out_r1/out_r2 the strings are rendered on the GPU (slots of len1+len2+1 bytes at ops_off[k])
 * and the op codes stay on the device; with cg neither comes down: CIGAR words and statistics do */
static int align_host(at_handle *h, int mode, int64_t npairs, const uint8_t *seq_blob,
                      const int64_t *off1, const int32_t *len1, const int64_t *off2, const int32_t *len2,
                      int want_traceback,
                      int32_t *out_score, int32_t *out_end_i, int32_t *out_end_j, int32_t *out_state,
                      uint8_t *out_ops, const int64_t *ops_off, int32_t *out_nops, char *out_r1, char *out_r2,
                      int64_t pair_base = 0,   /* index of pair 0 in the caller's batch, for messages */
                      const CigarReq *cg = nullptr)
{
	if (!h) return fail(nullptr, AT_ERR_ARG, "at_align_batch: NULL handle");
	if (mode < AT_MODE_GLOBAL || mode > AT_MODE_EDIT) return fail(h, AT_ERR_ARG, "unknown mode %d", mode);
	if (npairs < 0) return fail(h, AT_ERR_ARG, "negative npairs");
	if (npairs == 0) return AT_OK;
	if (!seq_blob || !off1 || !len1 || !off2 || !len2 || !out_score) return fail(h, AT_ERR_ARG, "NULL argument");
	if (mode == AT_MODE_EDIT && h->edit_infix && h->comm)
		return fail(h, AT_ERR_DOMAIN, "edit infix mode: one GPU only (this handle belongs to a multi-process job)");
	const bool tb = want_traceback && (mode != AT_MODE_EDIT || h->edit_tb);
	const bool strings = out_r1 != nullptr, cigar = cg != nullptr;
	if (tb && ((!out_ops && !strings && !cigar) || !ops_off || !out_nops)) return fail(h, AT_ERR_ARG, "traceback wanted but ops buffers are NULL");

	int max1 = 0, max2 = 0;
	bool uniform = true;
	int64_t ops_total = 0, ops_lo = INT64_MAX, blob_lo = INT64_MAX, slots_total = 0;
	for (int64_t k = 0; k < npairs; ++k) {
		if (len1[k] < 0 || len2[k] < 0) return fail(h, AT_ERR_ARG, "pair %lld: negative length", (long long)(pair_base + k));
		/* the domain on which the reference is defined (last paragraph) */
		if (mode == AT_MODE_FIT && len1[k] > len2[k])
			return fail(h, AT_ERR_FIT_ORDER, "first sequence must be shorter than the second");
		if (mode == AT_MODE_LOCAL && (len1[k] < 1 || len2[k] < 1)) return fail(h, AT_ERR_DOMAIN, "pair %lld: local needs non-empty sequences", (long long)(pair_base + k));
		if (mode == AT_MODE_FIT && len1[k] < 1) return fail(h, AT_ERR_DOMAIN, "pair %lld: fit needs a non-empty read", (long long)(pair_base + k));
		if (mode == AT_MODE_OVERLAP && len2[k] < 1) return fail(h, AT_ERR_DOMAIN, "pair %lld: overlap needs a non-empty second sequence", (long long)(pair_base + k));
		max1 = std::max(max1, len1[k]); max2 = std::max(max2, len2[k]);
		if (len1[k] != len1[0] || len2[k] != len2[0]) uniform = false;
		if (tb) {
			if (ops_off[k] < 0) return fail(h, AT_ERR_ARG, "pair %lld: negative ops offset", (long long)(pair_base + k));
			ops_total = std::max<int64_t>(ops_total, ops_off[k] + len1[k] + len2[k] + (strings ? 1 : 0));
			ops_lo = std::min<int64_t>(ops_lo, ops_off[k]);
			slots_total += (int64_t)len1[k] + len2[k];
		}
		if (off1[k] < 0 || off2[k] < 0) return fail(h, AT_ERR_ARG, "pair %lld: negative sequence offset", (long long)(pair_base + k));
		blob_lo = std::min<int64_t>(blob_lo, std::min(off1[k], off2[k]));
	}
	htrace("chunk: lengths checked, pair", pair_base);
	/* only the span of the blob and of the ops buffer that this call touches travels (a chunk of a larger batch,
	 * see at_align_batch, addresses the caller's buffers with absolute offsets) */
	if (!tb) ops_lo = 0;
	ops_total -= ops_lo;
	HIP_TRY(h, hipSetDevice(h->device));
	drop_stale_error();

	/* ---- inputs go up RAW; packing happens on the GPU (at_pack.hip.h).  Host work is O(npairs): one pass writes every descriptor
	 * ---- array into ONE page-locked block that mirrors the device block, so all of them travel in one copy; the raw bytes are
	 * ---- staged through page-locked memory in pieces by this thread (the chunks of a batch run on threads of their own: their
	 * ---- staging copies run side by side, where the runtime's own pageable path took them one after the other) ---- */
	auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
	const size_t n = (size_t)npairs;
	/* descriptor block, uploaded: soff[2n] swoff[2n] opsoff[n] (int64) slen[2n] (int32) -- per SEQUENCE, s1 of pair k at 2k, s2 at 2k + 1;
	 * behind it, made on the device (at_split_desc): woff1[n] woff2[n] (int64) len1[n] len2[n] (int32), what the sweep kernels take.
	 * The word offsets for byte words wait in page-locked memory in case a batch turns out not to be pure ACGT. */
	const size_t o_soff = 0, o_sw = o_soff + al(2 * n * 8), o_ops = o_sw + al(2 * n * 8), o_slen = o_ops + al(n * 8), up_bytes = o_slen + al(2 * n * 4);
	const size_t o_w1 = up_bytes, o_w2 = o_w1 + al(n * 8), o_l1 = o_w2 + al(n * 8), o_l2 = o_l1 + al(n * 4), desc_bytes = o_l2 + al(n * 4);
	int rc = grow_pinned(h, &h->hp_desc, &h->hp_desc_bytes, up_bytes + al(2 * n * 8));
	if (rc) return rc;
	char *hd = (char *)h->hp_desc;
	int64_t *p_soff = (int64_t *)(hd + o_soff), *p_sw = (int64_t *)(hd + o_sw), *p_ops = (int64_t *)(hd + o_ops), *p_sw8 = (int64_t *)(hd + up_bytes);
	int32_t *p_slen = (int32_t *)(hd + o_slen);
	const bool force8 = !scores_fit_byte(h, mode);    /* large scores: byte-compare kernels */
	int64_t nwords2 = 0, nwords8 = 0, blob_bytes = 0;
	for (int64_t k = 0; k < npairs; ++k) {
		const int a1 = len1[k], a2 = len2[k];
		p_soff[2 * k] = off1[k] - blob_lo; p_soff[2 * k + 1] = off2[k] - blob_lo;
		p_slen[2 * k] = a1; p_slen[2 * k + 1] = a2;
		p_sw[2 * k] = nwords2; nwords2 += (a1 + 15) / 16 + 1;
		p_sw[2 * k + 1] = nwords2; nwords2 += (a2 + 15) / 16 + 1;
		p_sw8[2 * k] = nwords8; nwords8 += (a1 + 3) / 4 + 1;
		p_sw8[2 * k + 1] = nwords8; nwords8 += (a2 + 3) / 4 + 1;
		blob_bytes = std::max<int64_t>(blob_bytes, std::max(p_soff[2 * k] + a1, p_soff[2 * k + 1] + a2));
		if (tb) p_ops[k] = ops_off[k] - ops_lo;
	}
	if (force8) memcpy(p_sw, p_sw8, 2 * n * 8);
	const int64_t nwords_max = std::max(nwords2, nwords8) + 4;
	/* device input block: words | descriptor block | flag | raw blob */
	const size_t b_words = al((size_t)nwords_max * 4), b_blob = al((size_t)blob_bytes + 32);   /* (at_pack reads whole dwords: up to 20 bytes behind the last base) */
	rc = grow(h, &h->d_in, &h->in_bytes, b_words + desc_bytes + 256 + b_blob);
	if (rc) return rc;
	char *din = (char *)h->d_in, *dd = din + b_words;
	uint32_t *d_words = (uint32_t *)din;
	int64_t *d_soff = (int64_t *)(dd + o_soff), *d_swoff = (int64_t *)(dd + o_sw), *d_opsoff = (int64_t *)(dd + o_ops);
	int64_t *d_woff1 = (int64_t *)(dd + o_w1), *d_woff2 = (int64_t *)(dd + o_w2);
	int32_t *d_slen = (int32_t *)(dd + o_slen), *d_len1 = (int32_t *)(dd + o_l1), *d_len2 = (int32_t *)(dd + o_l2);
	int *d_flag = (int *)(dd + desc_bytes);
	uint8_t *d_blob = (uint8_t *)(dd + desc_bytes + 256);
	hipStream_t s = h->stream;
	/* a caller whose sequences already lie in page-locked memory (hipHostMalloc / hipHostRegister) is copied from in place */
	bool caller_pinned = false;
	{
		hipPointerAttribute_t pattr;
		if (hipPointerGetAttributes(&pattr, seq_blob + blob_lo) == hipSuccess) caller_pinned = pattr.type == hipMemoryTypeHost;
		else (void)hipGetLastError();                  /* (ordinary memory: not an error) */
		if (env_ll("AT_HOST_NO_PINNED_CALLER", 0)) caller_pinned = false;
	}
	const uint8_t *up_src = seq_blob + blob_lo;
	if (!caller_pinned) {
		rc = grow_pinned(h, &h->hp_blob, &h->hp_blob_bytes, (size_t)blob_bytes + 64);
		if (rc) return rc;
	}
	/* (Tried and dropped, twice: the chunks of a batch uploading in order -- own streams chained by events, or one copy stream with
	 * the threads waiting on the host for their own copies -- so that each crosses the link at its full rate and the first sweep
	 * starts early.  Round 2: 2.28 / 2.37 ms per 100k pairs of C2 against 2.17 side by side.  Round 3, medians of 50 calls on one box:
	 * 1.90-2.12 ms against 1.99-2.04 with tracebacks, and 1.65-1.77 against 1.21-1.37 scores only -- copies queued side by side on six
	 * streams move more bytes per second than the same copies one behind the other.) */
	HIP_TRY(h, hipMemcpyAsync(dd, hd, up_bytes, hipMemcpyHostToDevice, s));
	/* pure-ACGT batches are packed HERE, while they are staged: the words go up (a quarter of the bytes), the raw blob and the GPU's
	 * packing kernel are skipped.  The first byte that is not ACGT ends the attempt: the raw path below takes the whole chunk. */
	bool host_packed = false;
	int up_pieces = 0;                                 /* (at_last_config: how the bytes went up) */
	if (!force8 && !caller_pinned && host_pack_available() && env_ll("AT_HOST_PACK", 1)) {
		rc = grow_pinned(h, &h->hp_blob, &h->hp_blob_bytes, (size_t)(nwords2 + 4) * 4 + 64);
		if (rc) return rc;
		uint32_t *hw = (uint32_t *)h->hp_blob;
		const int64_t piece_words = std::max<long long>(4096, env_ll("AT_HOST_STAGE_PIECE", 4 << 20)) / 16;   /* (a quarter of the raw pieces' bytes) */
		int64_t sent = 0;
		bool ok = true;
		for (int64_t k = 0; k < 2 * npairs && ok; ++k) {
			ok = pack2_avx2(up_src + p_soff[k], p_slen[k], hw + p_sw[k]);
			const int64_t done = k + 1 < 2 * npairs ? p_sw[k + 1] : nwords2;
			if (ok && (done - sent >= piece_words || k + 1 == 2 * npairs)) {
				if (k + 1 == 2 * npairs) for (int x = 0; x < 4; ++x) hw[nwords2 + x] = 0;
				const int64_t upto = k + 1 == 2 * npairs ? nwords2 + 4 : done;
				HIP_TRY(h, hipMemcpyAsync(d_words + sent, hw + sent, (size_t)(upto - sent) * 4, hipMemcpyHostToDevice, s));
				sent = upto;
				++up_pieces;
			}
		}
		host_packed = ok;
		if (!ok) { HIP_TRY(h, hipStreamSynchronize(s)); up_pieces = 0; }     /* (hp_blob is about to be reused for the raw bytes) */
	}
	if (host_packed) {
	} else if (caller_pinned) HIP_TRY(h, hipMemcpyAsync(d_blob, up_src, (size_t)blob_bytes, hipMemcpyHostToDevice, s));
	else {
		/* pieces of 4 MB: the staging of one beside the transfer of the one before (copies of 1 MB cross the link at 32 GB/s,
		 * of 5 MB at 50: tools/pcie_rate.py) */
		const size_t piece = (size_t)std::max<long long>(4096, env_ll("AT_HOST_STAGE_PIECE", 4 << 20));
		for (size_t at = 0; at < (size_t)blob_bytes; at += piece) {
			const size_t nb = std::min(piece, (size_t)blob_bytes - at);
			memcpy((char *)h->hp_blob + at, up_src + at, nb);
			HIP_TRY(h, hipMemcpyAsync(d_blob + at, (char *)h->hp_blob + at, nb, hipMemcpyHostToDevice, s));
			++up_pieces;
		}
	}
	at::PackArgs pa;
	pa.nseq = 2 * npairs; pa.blob = d_blob; pa.off = (const long long *)d_soff; pa.len = d_slen;
	pa.woff = (const long long *)d_swoff; pa.words = d_words; pa.not_acgt = d_flag;
	const unsigned pgrid = (unsigned)std::min<int64_t>((2 * npairs + 15) / 16, 8LL * h->ncu);
	int bits = force8 ? 8 : 2;
	int *p_flag = (int *)((char *)h->hp_flag);
	bool flag_pending = false;
	if (bits == 2 && !host_packed) {
		HIP_TRY(h, hipMemsetAsync(d_flag, 0, 4, s));
		hipLaunchKernelGGL(at::at_pack<2>, dim3(pgrid), dim3(256), 0, s, pa);
		HIP_TRY(h, hipMemcpyAsync(p_flag, d_flag, 4, hipMemcpyDeviceToHost, s));
		flag_pending = true;
	}
	htrace("chunk: uploads and packing queued, pair", pair_base);
	/* The alphabet of the batch is known when the packing kernel's flag is down -- one wait for the uploads per chunk.  A ragged
	 * batch makes its plan (frames, the order of the pairs: host work over the lengths alone) BEFORE that wait, for the 2-bit
	 * alphabet it expects, and again only if the flag says otherwise. */
	auto settle_alphabet = [&]() -> int {
		if (flag_pending) {
			HIP_TRY(h, hipStreamSynchronize(s));
			htrace("chunk: packed, pair", pair_base);
			flag_pending = false;
			if (*p_flag) {                                 /* some byte is not one of ACGT: byte words, byte kernels */
				bits = 8;
				HIP_TRY(h, hipMemcpyAsync(d_swoff, p_sw8, 2 * n * 8, hipMemcpyHostToDevice, s));
			}
		}
		if (bits == 8) hipLaunchKernelGGL(at::at_pack<8>, dim3(pgrid), dim3(256), 0, s, pa);
		hipLaunchKernelGGL(at::at_split_desc, dim3((unsigned)std::min<int64_t>((npairs + 255) / 256, 8LL * h->ncu)), dim3(256), 0, s,
		                   (const long long *)d_swoff, (const int *)d_slen, (long long)npairs, (long long *)d_woff1, (long long *)d_woff2, d_len1, d_len2);
		HIP_TRY(h, hipGetLastError());
		return AT_OK;
	};
	const size_t b_len1 = al((size_t)npairs * 4);
	/* device output block: score | end_i | end_j | state | nops | ops */
	const size_t b_ops = al((size_t)ops_total + 64), b_pfx = al((size_t)(npairs + 1) * 8);
	const size_t out_need = 5 * b_len1 + b_ops + (tb ? b_pfx : 0);
	rc = grow(h, &h->d_out, &h->out_bytes, out_need);
	if (rc) return rc;
	char *dout = (char *)h->d_out;
	int32_t *d_score = (int32_t *)dout, *d_ei = (int32_t *)(dout + b_len1), *d_ej = (int32_t *)(dout + 2 * b_len1);
	int32_t *d_st = (int32_t *)(dout + 3 * b_len1), *d_nops = (int32_t *)(dout + 4 * b_len1);
	uint8_t *d_ops = (uint8_t *)(dout + 5 * b_len1);
	int64_t *d_poff = (int64_t *)(dout + 5 * b_len1 + b_ops);   /* exclusive prefix sums of nops (tb only) */

	/* ragged batch.  Affine alignments of reads whose scores stay within 16 bits (and overlap with tracebacks) go to the packed kernels
	 * in FRAMES (RAG kernels): a work item sweeps the extents its alignments need and every alignment keeps its own.  The order of the
	 * pairs and the launches are at_ragplan.h's; everything else runs on the int32 kernel, pairs handed out largest first. */
	int *d_order = nullptr;
	bool frames = false;
	/* a launch over this chunk's descriptors and results: n pairs of at most m1 x m2 */
	auto chunk_req = [&](int64_t n, int32_t m1, int32_t m2) {
		BatchReq q(h);
		q.mode = mode; q.npairs = n; q.d_seq = d_words; q.bits = bits; q.stream = s;
		q.d_woff1 = d_woff1; q.d_len1 = d_len1; q.d_woff2 = d_woff2; q.d_len2 = d_len2; q.max_len1 = m1; q.max_len2 = m2;
		q.want_traceback = tb ? 1 : 0;
		q.d_score = d_score; q.d_end_i = d_ei; q.d_end_j = d_ej; q.d_state = d_st;
		if (tb) { q.d_ops = d_ops; q.d_ops_off = d_opsoff; q.d_nops = d_nops; }
		return q;
	};
	const bool ragged = !uniform && npairs > 1 && npairs < (1LL << 31);
	if (!ragged) {
		rc = settle_alphabet();
		if (rc) return rc;
	}
	if (ragged) {
		int th = 0, min1 = INT32_MAX, min2 = INT32_MAX;
		for (int64_t k = 0; k < npairs; ++k) { min1 = std::min(min1, len1[k]); min2 = std::min(min2, len2[k]); }
		const bool affine = mode == AT_MODE_LOCAL || mode == AT_MODE_GLOBAL || mode == AT_MODE_FIT;
		const bool ovl = mode == AT_MODE_OVERLAP && tb;
		const int kmode_f = mode == AT_MODE_LOCAL ? at::K_LOCAL : mode == AT_MODE_GLOBAL ? at::K_GLOBAL : mode == AT_MODE_OVERLAP ? at::K_OVERLAP
		                  : h->use_jump ? at::K_FITJ : at::K_FIT;
		/* (a bucket of a local batch is a launch, and the launches of a chunk follow each other on its stream: 4 096 pairs per bucket and
		 * 33k-pair chunks made up to eight launches per class -- 30..150-base reads 2.24 ms per 100k pairs, 1.92-1.96 with at most two) */
		const int64_t min_bucket = env_ll("AT_RAGGED_MIN_BUCKET", 16384);
		at::RagPlan plan;
		for (int pass = 0; pass < 2; ++pass) {   /* (the second pass: the batch was not pure ACGT after all) */
			const int planned_bits = bits;
			/* frames: every read within the mode's longest one-strip frame (at_classes.h), scores within 16 bits */
			frames = (affine || ovl) && max1 <= at::one_strip_top(mode) && min1 >= 1 && min2 >= 1 && npairs >= 64 && env_ll("AT_RAGGED_PACKED", 1) &&
			         packed_ok(h, mode, bits, max1, max2, ovl ? 2 : 4, &th);
			/* every frame is at most max1 x max2: if a group width has no packed kernel for that (s2 too long for LDS), none is tried */
			if (frames) {
				const bool hasj = kmode_f == at::K_FITJ;
				const int tsf = ovl ? 2 : 4;
				int prev = -1;
				for (int gq : at::kRagGroups) {
					const int l1q = std::min(max1, at::rag_group_top(gq));   /* the longest read of the batch on that width */
					if (!frames || (ovl && gq != 64) || l1q < min1 || l1q == prev) continue;
					prev = l1q;
					const at::GroupRows c = at::rag_class(mode, ovl, l1q);
					frames = packed16_kernel_exists(kmode_f, layout16_for(tb, hasj, l1q, max2, tsf, c.g, ovl, kmode_f, ovl ? c.k : 0), tb, tsf, bits, c.g);
				}
			}
			plan = at::rag_plan(mode, ovl, len1, len2, npairs, max1, max2, min_bucket, frames);
			if (pass == 0) {
				rc = settle_alphabet();
				if (rc) return rc;
			}
			if (bits == planned_bits) break;
		}
		htrace("chunk: planned, pair", pair_base);
		/* the order goes up from page-locked memory: nothing to wait for on the host */
		const std::vector<int> &order = plan.order;
		rc = grow(h, &h->d_order, &h->order_bytes, order.size() * 4);
		if (rc) return rc;
		rc = grow_pinned(h, &h->hp_order, &h->hp_order_bytes, order.size() * 4);
		if (rc) return rc;
		memcpy(h->hp_order, order.data(), order.size() * 4);
		d_order = (int *)h->d_order;
		HIP_TRY(h, hipMemcpyAsync(d_order, h->hp_order, order.size() * 4, hipMemcpyHostToDevice, s));
		for (const at::RagLaunch &L : plan.launches) {
			BatchReq fr = chunk_req(L.b1 - L.b0, L.f1, L.f2);
			fr.d_order = d_order + L.b0; fr.rag = L.g;
			rc = align_device(h, fr);
			if (rc) return rc;
		}
		if (frames) cfg_append(h, mode == AT_MODE_LOCAL ? " (%d frames)" : " (%d frames, equal-l1 work items)", (int)plan.launches.size());
	}
	if (!frames) {
		BatchReq br = chunk_req(npairs, max1, max2);
		br.uniform_shape = uniform ? 1 : 0; br.d_order = d_order;
		rc = align_device(h, br);
		if (rc) return rc;
	}
	htrace("chunk: sweep queued, pair", pair_base);
	{
		char note[96];
		if (host_packed) snprintf(note, sizeof note, " [upload: 2-bit words packed on the host, %d pieces]", up_pieces);
		else if (caller_pinned) snprintf(note, sizeof note, " [upload: raw bytes from the caller's page-locked memory]");
		else snprintf(note, sizeof note, " [upload: raw bytes staged, %d pieces]", up_pieces);
		cfg_append(h, "%s", note);
	}
	/* ---- results: the five fixed-size arrays come down in ONE copy into page-locked memory.  Only the bytes of each pair's own
	 * ---- traceback travel and are written: the used part of every ops slot (or string slot) is packed back to back on the GPU and
	 * ---- comes down with the same synchronisation -- as many bytes as the previous call's payload suggests, the rest (if this
	 * ---- batch's tracebacks are longer) behind a second one -- and is scattered into the caller's slots here.  Bytes of the
	 * ---- caller's buffers between and behind the slots are never touched, whatever order the slots are in. ---- */
	const size_t res_bytes = 5 * b_len1;
	const size_t b_str = al((size_t)slots_total + (size_t)npairs + 64);
	const size_t pk_cap = tb && !cigar ? (strings ? 2 : 1) * b_str : 0;
	rc = grow_pinned(h, &h->hp_out, &h->hp_out_bytes, res_bytes + 64 + (tb ? b_pfx : 0) + pk_cap);
	if (rc) return rc;
	char *ho = (char *)h->hp_out;
	int *p_rflag = (int *)(ho + res_bytes);
	int64_t *h_poff = (int64_t *)(ho + res_bytes + 64);
	char *h_pk1 = ho + res_bytes + 64 + (tb ? b_pfx : 0), *h_pk2 = h_pk1 + b_str;
	HIP_TRY(h, hipMemcpyAsync(ho, dout, res_bytes, hipMemcpyDeviceToHost, s));
	*p_rflag = 0;
	uint8_t *d_pk1 = nullptr, *d_pk2 = nullptr;
	size_t spec = 0;                                   /* payload bytes fetched before the total is known */
	/* the CIGAR form: counts | statistics | words in one device block; counts and statistics come down in one copy, the offsets in a
	 * second, and as many words as the previous call's payload suggests in a third */
	const size_t c_head = al(n * 4) + al(n * 32), c_pfx = al((n + 1) * 8);
	size_t spec_w = 0;
	if (cigar) {
		rc = grow(h, &h->d_cg, &h->cg_bytes, c_head + (size_t)slots_total * 4 + 64);
		if (rc) return rc;
		char *dc = (char *)h->d_cg;
		rc = at_cigar_batch_device(h, npairs, d_words, bits, d_woff1, d_woff2, d_ei, d_ej, d_ops, d_opsoff, d_nops, cg->flags,
		                           (int32_t *)dc, (int32_t *)(dc + al(n * 4)), d_poff, (uint32_t *)(dc + c_head), slots_total, s);
		if (rc) return rc;
		cfg_append(h, " [cigar: %d lanes per pair]", h->last_cigar_lanes);
		/* (the guess is the ops form's, not a measurement of this one: the last batch's payload per pair and a quarter more, and the
		 * same 64 KiB floor; a handle's first batch assumes four runs per pair) */
		spec_w = std::min<size_t>((size_t)slots_total, (size_t)(h->last_cigar_per_pair * 1.25 * (double)npairs) + 16384);
		rc = grow_pinned(h, &h->hp_cg, &h->hp_cg_bytes, c_head + c_pfx + spec_w * 4);
		if (rc) return rc;
		char *hc = (char *)h->hp_cg;
		HIP_TRY(h, hipMemcpyAsync(hc, dc, c_head, hipMemcpyDeviceToHost, s));
		HIP_TRY(h, hipMemcpyAsync(hc + c_head, d_poff, (size_t)(npairs + 1) * 8, hipMemcpyDeviceToHost, s));
		if (spec_w) HIP_TRY(h, hipMemcpyAsync(hc + c_head + c_pfx, dc + c_head, spec_w * 4, hipMemcpyDeviceToHost, s));
	}
	if (tb && !cigar) {
		rc = grow(h, &h->d_str, &h->str_bytes, (strings ? 2 : 1) * b_str + (strings ? b_pfx : 0));
		if (rc) return rc;
		d_pk1 = (uint8_t *)h->d_str; d_pk2 = d_pk1 + b_str;
		if (!strings) {
			rc = at_compact_ops_device(h, npairs, d_ops, d_opsoff, d_nops, d_pk1, slots_total, d_poff, s);
			if (rc) return rc;
		} else {
			rc = scan_nops_device(h, npairs, d_nops, d_poff, s);
			if (rc) return rc;
			int64_t *d_stroff = (int64_t *)(d_pk1 + 2 * b_str);   /* string k starts at poff[k] + k: one NUL behind each */
			hipLaunchKernelGGL(at::at_add_index, dim3((unsigned)std::min<int64_t>((npairs + 255) / 256, 8LL * h->ncu)), dim3(256), 0, s,
			                   (const long long *)d_poff, (long long *)d_stroff, (long long)npairs);
			HIP_TRY(h, hipMemsetAsync(h->d_rflag, 0, 4, s));
			rc = at_render_batch_device(h, npairs, d_words, bits, d_woff1, d_woff2, d_ei, d_ej, d_ops, d_opsoff, d_nops,
			                            d_pk1, d_pk2, d_stroff, 1, s);
			if (rc) return rc;
			cfg_append(h, " [strings: %d lanes per pair]", h->last_render_lanes);
			HIP_TRY(h, hipMemcpyAsync(p_rflag, h->d_rflag, 4, hipMemcpyDeviceToHost, s));
		}
		HIP_TRY(h, hipMemcpyAsync(h_poff, d_poff, (size_t)(npairs + 1) * 8, hipMemcpyDeviceToHost, s));
		spec = std::min<size_t>((size_t)slots_total + (strings ? (size_t)npairs : 0),
		                        (size_t)((double)h->last_payload_per_pair * 1.25 * (double)npairs) + 65536);
		HIP_TRY(h, hipMemcpyAsync(h_pk1, d_pk1, spec, hipMemcpyDeviceToHost, s));
		if (strings) HIP_TRY(h, hipMemcpyAsync(h_pk2, d_pk2, spec, hipMemcpyDeviceToHost, s));
	}
	HIP_TRY(h, hipStreamSynchronize(s));
	htrace("chunk: results down, pair", pair_base);
	const int32_t *r_score = (const int32_t *)ho, *r_nops = (const int32_t *)(ho + 4 * b_len1);
	for (int64_t k = 0; k < npairs; ++k) {
		if (r_score[k] == INT32_MIN || (tb && r_nops[k] < 0))
			return fail(h, AT_ERR_DOMAIN, "pair %lld: input outside the domain on which the reference is defined", (long long)(pair_base + k));
	}
	memcpy(out_score, ho, (size_t)npairs * 4);
	if (out_end_i) memcpy(out_end_i, ho + b_len1, (size_t)npairs * 4);
	if (out_end_j) memcpy(out_end_j, ho + 2 * b_len1, (size_t)npairs * 4);
	if (out_state) memcpy(out_state, ho + 3 * b_len1, (size_t)npairs * 4);
	if (cigar) {
		memcpy(out_nops, r_nops, (size_t)npairs * 4);
		const char *hc = (const char *)h->hp_cg;
		const int32_t *r_nc = (const int32_t *)hc;
		const int64_t *r_off = (const int64_t *)(hc + c_head);
		const int64_t total = r_off[(size_t)npairs];
		if (total < 0 || total > slots_total) return fail(h, AT_ERR_DOMAIN, "CIGAR lengths inconsistent with the slots");
		for (int64_t k = 0; k < npairs; ++k)
			if (r_nc[k] < 0) return fail(h, AT_ERR_DOMAIN, "pair %lld: traceback inconsistent with its sequences", (long long)(pair_base + k));
		memcpy(cg->out_ncigar, r_nc, (size_t)npairs * 4);
		memcpy(cg->out_stats, hc + al(n * 4), (size_t)npairs * 32);
		memcpy(cg->out_off, r_off, (size_t)npairs * 8);
		h->last_cigar_per_pair = (double)total / (double)npairs;
		if ((size_t)total > spec_w) {       /* more runs than the last batch's: the rest of the payload, as the other two forms do */
			const size_t need = c_head + c_pfx + (size_t)total * 4;
			if (need > h->hp_cg_bytes) {    /* ... into a larger buffer; the words that are down already move over */
				void *nb = nullptr;
				size_t nbytes = 0;
				rc = grow_pinned(h, &nb, &nbytes, need);
				if (rc) return rc;
				memcpy((char *)nb + c_head + c_pfx, (const char *)h->hp_cg + c_head + c_pfx, spec_w * 4);
				(void)hipHostFree(h->hp_cg);
				h->hp_cg = nb; h->hp_cg_bytes = nbytes;
			}
			HIP_TRY(h, hipMemcpyAsync((char *)h->hp_cg + c_head + c_pfx + spec_w * 4, (const char *)h->d_cg + c_head + spec_w * 4,
			                          ((size_t)total - spec_w) * 4, hipMemcpyDeviceToHost, s));
			HIP_TRY(h, hipStreamSynchronize(s));
		}
		h->cg_words = (const uint32_t *)((const char *)h->hp_cg + c_head + c_pfx);
		h->cg_total = total;
	}
	if (tb && !cigar) {
		memcpy(out_nops, r_nops, (size_t)npairs * 4);
		const int64_t total = h_poff[(size_t)npairs];
		if (total < 0 || total > slots_total) return fail(h, AT_ERR_DOMAIN, "traceback lengths inconsistent with the slots");
		const size_t have = (size_t)total + (strings ? (size_t)npairs : 0);
		h->last_payload_per_pair = (double)have / (double)npairs;
		if (have > spec) {       /* longer tracebacks than the last batch's: the rest of the payload */
			HIP_TRY(h, hipMemcpyAsync(h_pk1 + spec, d_pk1 + spec, have - spec, hipMemcpyDeviceToHost, s));
			if (strings) HIP_TRY(h, hipMemcpyAsync(h_pk2 + spec, d_pk2 + spec, have - spec, hipMemcpyDeviceToHost, s));
			HIP_TRY(h, hipStreamSynchronize(s));
		}
		if (!strings) {
			for (int64_t k = 0; k < npairs; ++k)
				if (r_nops[k] > 0) memcpy(out_ops + ops_off[k], h_pk1 + h_poff[(size_t)k], (size_t)r_nops[k]);
		} else {
			for (int64_t k = 0; k < npairs; ++k) {
				const size_t src = (size_t)(h_poff[(size_t)k] + k), nb = (size_t)r_nops[k] + 1;   /* with the NUL */
				memcpy(out_r1 + ops_off[k], h_pk1 + src, nb);
				memcpy(out_r2 + ops_off[k], h_pk2 + src, nb);
			}
		}
	}
	if (*p_rflag) return fail(h, AT_ERR_DOMAIN, "traceback inconsistent with its sequences");
	htrace("chunk: done, pair", pair_base);
	return AT_OK;
}

/* A large batch is cut into contiguous chunks that run side by side, each on its own handle (stream, workspace) and
 * host thread: the upload of one chunk, the sweep of another and the download of a third overlap, and the launches fill
 * each other's tails.  Chunks address the caller's buffers with the caller's absolute offsets. */
static int align_host_mt(at_handle *h, int mode, int64_t npairs, const uint8_t *seq_blob,
                         const int64_t *off1, const int32_t *len1, const int64_t *off2, const int32_t *len2,
                         int want_traceback,
                         int32_t *out_score, int32_t *out_end_i, int32_t *out_end_j, int32_t *out_state,
                         uint8_t *out_ops, const int64_t *ops_off, int32_t *out_nops, char *out_r1, char *out_r2,
                         const CigarReq *cg = nullptr, uint32_t *out_cigar = nullptr, int64_t cigar_cap = 0)
{
	/* the CIGAR form, behind the join: chunk c's words lie in its handle's page-locked buffer and its offsets count from its own
	 * first pair.  The payloads go back to back in pair order into the caller's buffer -- of a chunk that crosses the capacity, the
	 * pairs that end within it -- and the offsets become the batch's (out_off[npairs] = total words) */
	auto cigar_gather = [&](int nch, int64_t per_chunk) {
		int64_t base = 0;
		for (int c = 0; c < nch; ++c) {
			const int64_t lo = std::min<int64_t>(npairs, c * per_chunk), nn = std::min<int64_t>(npairs, lo + per_chunk) - lo;
			if (nn <= 0) continue;
			const at_handle *hh = c == 0 ? h : h->kids[(size_t)c - 1];
			int64_t fit = 0;               /* words of the chunk's leading pairs that end within the capacity */
			for (int64_t k = 0; k < nn; ++k) {
				const int64_t end = base + cg->out_off[lo + k] + cg->out_ncigar[lo + k];
				if (end <= cigar_cap) fit = end - base;
				cg->out_off[lo + k] += base;
			}
			if (fit > 0) memcpy(out_cigar + base, hh->cg_words, (size_t)fit * 4);
			base += hh->cg_total;
		}
		cg->out_off[npairs] = base;
	};
	/* uniform batches: six chunks (100k pairs of C2: 3.37 ms in one piece, 2.49 in 3 chunks, 2.28 in 6); ragged ones, whose chunks are
	 * sorted into frames one by one: three (fit -s 100..150 x 400..500: 785 GCUPS in 3 chunks, 693 in 6 -- smaller frames) */
	htrace("batch: enter, pairs", npairs);
	bool same = len1 && len2;
	for (int64_t k = 1; same && k < npairs; ++k) same = len1[k] == len1[0] && len2[k] == len2[0];
	const long long want = env_ll("AT_HOST_CHUNKS", same ? 6 : 3);
	const long long min_pairs = env_ll("AT_HOST_CHUNK_MIN", 16384);
	int nchunks = (int)std::max<long long>(1, std::min<long long>(want, 12));
	if (!h || npairs < 2 * min_pairs || !seq_blob || !off1 || !len1 || !off2 || !len2 || !out_score) nchunks = 1;
	else nchunks = (int)std::min<long long>(nchunks, npairs / min_pairs);
	if (nchunks <= 1 && !cg)
		return align_host(h, mode, npairs, seq_blob, off1, len1, off2, len2, want_traceback, out_score, out_end_i, out_end_j,
		                  out_state, out_ops, ops_off, out_nops, out_r1, out_r2);
	if (nchunks <= 1) {
		const int rc = align_host(h, mode, npairs, seq_blob, off1, len1, off2, len2, want_traceback, out_score, out_end_i, out_end_j,
		                          out_state, out_ops, ops_off, out_nops, out_r1, out_r2, 0, cg);
		if (rc == AT_OK && npairs > 0) cigar_gather(1, npairs);
		return rc;
	}
	while ((int)h->kids.size() < nchunks - 1) {
		at_handle *k = nullptr;
		const int dev = h->device;
		const int rc = at_init(&dev, 1, &k);
		if (rc) return fail(h, rc, "helper handle: %s", at_last_error(nullptr));
		h->kids.push_back(k);
	}
	for (int c = 0; c < nchunks - 1; ++c) {
		at_handle *k = h->kids[(size_t)c];
		k->edit_tb = h->edit_tb;
		k->edit_infix = h->edit_infix;
		if (k->m != h->m || k->u != h->u || k->o != h->o || k->e != h->e || k->j != h->j || k->use_jump != h->use_jump ||
		    k->sites != h->sites) {
			k->m = h->m; k->u = h->u; k->o = h->o; k->e = h->e; k->j = h->j; k->use_jump = h->use_jump; k->sites = h->sites;
			k->sitemask_dirty = true;
		}
	}
	std::vector<int> rcs((size_t)nchunks, AT_OK);
	/* (Tried: unequal chunks -- small first ones so that the GPU starts early, small last ones so that the tail behind the last upload is
	 * short: 1.95 .. 2.21 ms against 2.02 for equal shares; the box's noise.) */
	const int64_t per = ((npairs + nchunks - 1) / nchunks + 7) & ~(int64_t)7;
	auto run = [&](int c) {
		const int64_t lo = std::min<int64_t>(npairs, c * per), n = std::min<int64_t>(npairs, lo + per) - lo;
		at_handle *hh = c == 0 ? h : h->kids[(size_t)c - 1];
		if (n <= 0) return;
		/* (a chunk runs on a pool thread: an exception that left it would end the process in std::terminate) */
		CigarReq mine;
		if (cg) { mine.flags = cg->flags; mine.out_stats = cg->out_stats + 8 * lo; mine.out_ncigar = cg->out_ncigar + lo; mine.out_off = cg->out_off + lo; }
		rcs[(size_t)c] = guarded(hh, "at_align_batch", [&] {
			return align_host(hh, mode, n, seq_blob, off1 + lo, len1 + lo, off2 + lo, len2 + lo, want_traceback,
			                  out_score + lo, out_end_i ? out_end_i + lo : nullptr, out_end_j ? out_end_j + lo : nullptr,
			                  out_state ? out_state + lo : nullptr, out_ops, ops_off ? ops_off + lo : nullptr,
			                  out_nops ? out_nops + lo : nullptr, out_r1, out_r2, lo, cg ? &mine : nullptr);
		});
	};
	if (!h->pool) h->pool = new HostPool();
	h->pool->run(nchunks, run);
	for (int c = 0; c < nchunks; ++c) {
		if (rcs[(size_t)c] != AT_OK) {
			if (c > 0) snprintf(h->err, sizeof h->err, "%s", h->kids[(size_t)c - 1]->err);
			snprintf(g_err, sizeof g_err, "%s", h->err);
			return rcs[(size_t)c];
		}
	}
	if (cg) cigar_gather(nchunks, per);
	cfg_append(h, " x%d chunks", nchunks);
	return AT_OK;
}

/* ---- all-vs-all over one read set held in HOST memory ----
 * The reads go up once and are packed once (upload_reads); pairs of the strict upper triangle are enumerated on the GPU
 * (at_align_allpairs_device).  The triangle is swept in SLICES of at most `chunk` pairs, so device and host memory are
 * bounded by the slice, not by the 1.25e9 pairs of C5: scores and end cells of slice c come down on a copy stream and are
 * handed to the caller while the sweep of slice c + 1 runs. */
struct ReadSet {
	uint32_t *d_words = nullptr;
	int64_t *d_swoff = nullptr;
	int32_t *d_len = nullptr;
	int bits = 2, maxlen = 0;
};

/* pairs [first, first + n) of the triangle over the nreads reads of a set */
static BatchReq triangle_req(const at_handle *h, int mode, const ReadSet &rs, int64_t nreads, int64_t first, int64_t n, hipStream_t s)
{
	BatchReq r(h);
	r.mode = mode; r.npairs = n; r.d_seq = rs.d_words; r.bits = rs.bits; r.stream = s;
	r.d_woff1 = r.d_woff2 = rs.d_swoff; r.d_len1 = r.d_len2 = rs.d_len; r.max_len1 = r.max_len2 = rs.maxlen;
	r.ap_n = nreads; r.ap_first = first;
	return r;
}

/* hands out 256-byte-aligned typed sub-ranges of one buffer.  A function says its layout ONCE, as a function of a Carver, and carve()
 * runs it twice: without a base, where take() only counts -- the bytes asked of grow() -- and then on the buffer */
struct Carver {
	char *base = nullptr;
	size_t at = 0;
	template <typename T> T *take(size_t n) { T *p = base ? (T *)(base + at) : nullptr; at += (n * sizeof(T) + 255) & ~(size_t)255; return p; }
};

template <typename Layout>
static int carve(at_handle *h, void **buf, size_t *have, Layout &&layout)
{
	Carver count, c;
	layout(count);
	if (int rc = grow(h, buf, have, count.at)) return rc;
	c.base = (char *)*buf;
	layout(c);
	return AT_OK;
}

/* nrev > 0: the read set also gets, as reads nreads .. nreads + nrev - 1, the reverse complements of reads 0 .. nrev - 1, made on the
 * device from their packed words (at_revcomp.hip) behind the pack kernel: no byte goes up twice */
static int upload_reads(at_handle *h, int mode, int64_t nreads, const uint8_t *seq_blob, const int64_t *off, const int32_t *len, ReadSet *rs,
                        int64_t nrev = 0)
{
	int maxlen = 0;
	const int64_t ntot = nreads + nrev;
	int64_t blob_lo = INT64_MAX, blob_bytes = 0, nwords2 = 0, nwords8 = 0;
	std::vector<int64_t> soff((size_t)nreads), swoff2((size_t)ntot), swoff8((size_t)ntot);
	for (int64_t k = 0; k < nreads; ++k) {
		if (len[k] < 0 || off[k] < 0) return fail(h, AT_ERR_ARG, "read %lld: negative length or offset", (long long)k);
		if ((mode == AT_MODE_LOCAL || mode == AT_MODE_OVERLAP) && len[k] < 1) return fail(h, AT_ERR_DOMAIN, "read %lld: empty", (long long)k);
		maxlen = std::max(maxlen, len[k]);
		blob_lo = std::min(blob_lo, off[k]);
	}
	for (int64_t k = 0; k < nreads; ++k) {
		soff[(size_t)k] = off[k] - blob_lo;
		swoff2[(size_t)k] = nwords2; nwords2 += (len[k] + 15) / 16 + 1;
		swoff8[(size_t)k] = nwords8; nwords8 += (len[k] + 3) / 4 + 1;
		blob_bytes = std::max<int64_t>(blob_bytes, soff[(size_t)k] + len[k]);
	}
	for (int64_t k = 0; k < nrev; ++k) {
		swoff2[(size_t)(nreads + k)] = nwords2; nwords2 += (len[k] + 15) / 16 + 1;
		swoff8[(size_t)(nreads + k)] = nwords8; nwords8 += (len[k] + 3) / 4 + 1;
	}
	HIP_TRY(h, hipSetDevice(h->device));
	drop_stale_error();
	uint32_t *d_words = nullptr; int64_t *d_soff = nullptr, *d_swoff = nullptr; int32_t *d_len = nullptr; int *d_flag = nullptr; uint8_t *d_blob = nullptr;
	int rc = carve(h, &h->d_in, &h->in_bytes, [&](Carver &c) {
		d_words = c.take<uint32_t>((size_t)(std::max(nwords2, nwords8) + 4));
		d_soff = c.take<int64_t>((size_t)ntot); d_swoff = c.take<int64_t>((size_t)ntot);
		d_len = c.take<int32_t>((size_t)ntot);
		d_flag = c.take<int>(1);
		d_blob = c.take<uint8_t>((size_t)blob_bytes + 32);   /* (at_pack reads whole dwords: up to 20 bytes behind the last base) */
	});
	if (rc) return rc;
	hipStream_t s = h->stream;
	HIP_TRY(h, hipMemcpyAsync(d_blob, seq_blob + blob_lo, (size_t)blob_bytes, hipMemcpyHostToDevice, s));
	HIP_TRY(h, hipMemcpyAsync(d_soff, soff.data(), (size_t)nreads * 8, hipMemcpyHostToDevice, s));
	HIP_TRY(h, hipMemcpyAsync(d_len, len, (size_t)nreads * 4, hipMemcpyHostToDevice, s));
	if (nrev) HIP_TRY(h, hipMemcpyAsync(d_len + nreads, d_len, (size_t)nrev * 4, hipMemcpyDeviceToDevice, s));
	at::PackArgs pa;
	pa.nseq = nreads; pa.blob = d_blob; pa.off = (const long long *)d_soff; pa.len = d_len;
	pa.woff = (const long long *)d_swoff; pa.words = d_words; pa.not_acgt = d_flag;
	const unsigned pgrid = (unsigned)std::min<int64_t>((nreads + 15) / 16, 8LL * h->ncu);
	int bits = scores_fit_byte(h, mode) ? 2 : 8, flag = 0;
	if (bits == 2) {
		HIP_TRY(h, hipMemsetAsync(d_flag, 0, 4, s));
		HIP_TRY(h, hipMemcpyAsync(d_swoff, swoff2.data(), (size_t)ntot * 8, hipMemcpyHostToDevice, s));
		hipLaunchKernelGGL(at::at_pack<2>, dim3(pgrid), dim3(256), 0, s, pa);
		HIP_TRY(h, hipMemcpyAsync(&flag, d_flag, 4, hipMemcpyDeviceToHost, s));
		HIP_TRY(h, hipStreamSynchronize(s));
		if (flag) bits = 8;
	}
	if (bits == 8) {
		HIP_TRY(h, hipMemcpyAsync(d_swoff, swoff8.data(), (size_t)ntot * 8, hipMemcpyHostToDevice, s));
		hipLaunchKernelGGL(at::at_pack<8>, dim3(pgrid), dim3(256), 0, s, pa);
	}
	HIP_TRY(h, hipGetLastError());
	if (nrev) {
		at::RevcompArgs ra;
		ra.nseq = nrev; ra.seq = d_words; ra.woff = (const long long *)d_swoff; ra.len = d_len;
		ra.out = d_words; ra.out_woff = (const long long *)(d_swoff + nreads);   /* (the reverse reads' words lie behind every forward read's) */
		HIP_TRY(h, at_revcomp_launch(&ra, bits, h->ncu, s));
	}
	HIP_TRY(h, hipStreamSynchronize(s));   /* swoff* are stack-lifetime vectors */
	rs->d_words = d_words; rs->d_swoff = d_swoff; rs->d_len = d_len; rs->bits = bits; rs->maxlen = maxlen;
	return AT_OK;
}

static int check_allpairs_args(at_handle *h, const char *who, int mode, int64_t nreads, int64_t first_pair, int64_t npairs)
{
	if (!h) return fail(nullptr, AT_ERR_ARG, "%s: NULL handle", who);
	if (mode < AT_MODE_GLOBAL || mode > AT_MODE_EDIT) return fail(h, AT_ERR_ARG, "unknown mode %d", mode);
	if (mode == AT_MODE_FIT) return fail(h, AT_ERR_ARG, "all-vs-all: fit needs ordered lengths (l1 <= l2); use the pair list entry");
	if (mode == AT_MODE_EDIT && h->edit_infix) return fail(h, AT_ERR_DOMAIN, "edit infix mode: no all-vs-all (pair lists and searches only)");
	if (nreads < 2 || nreads >= (1LL << 31) || first_pair < 0 || npairs < 0 || first_pair + npairs > nreads * (nreads - 1) / 2)
		return fail(h, AT_ERR_ARG, "all-vs-all: pair range [%lld, +%lld) outside the %lld*(%lld-1)/2 ordered pairs",
		            (long long)first_pair, (long long)npairs, (long long)nreads, (long long)nreads);
	return AT_OK;
}

/* scores + end cells of pairs [first_pair, first_pair + npairs) in slices; fn(user, first pair of the slice, pairs, score, end_i,
 * end_j, state) sees every slice once, in order, on the calling thread */
static int allpairs_scores(at_handle *h, int mode, int64_t nreads, const ReadSet &rs, int64_t first_pair, int64_t npairs,
                           int64_t chunk, at_allpairs_chunk_fn fn, void *user)
{
	if (chunk <= 0) chunk = env_ll("AT_ALLPAIRS_CHUNK", 4LL << 20);
	chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, std::min<int64_t>(npairs, 1LL << 28)));
	auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
	const size_t b_res = al((size_t)chunk * 4);
	int rc = grow(h, &h->d_out, &h->out_bytes, 2 * 4 * b_res);
	if (rc) return rc;
	if (h->pin_bytes < 2 * 4 * b_res) {
		if (h->h_pin) { (void)hipHostFree(h->h_pin); h->h_pin = nullptr; h->pin_bytes = 0; }
		if (hipHostMalloc(&h->h_pin, 2 * 4 * b_res, hipHostMallocDefault) != hipSuccess) {
			h->h_pin = nullptr;
			(void)hipGetLastError();   /* (as in grow) */
			return fail(h, AT_ERR_NOMEM, "hipHostMalloc(%zu) for the result slices failed", 2 * 4 * b_res);
		}
		h->pin_bytes = 2 * 4 * b_res;
	}
	if (!h->copy_stream) HIP_TRY(h, hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
	for (int q = 0; q < 2; ++q) {
		if (!h->ev_sweep[q]) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_sweep[q], hipEventDisableTiming));
		if (!h->ev_copy[q]) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_copy[q], hipEventDisableTiming));
	}
	hipStream_t s = h->stream, cs = h->copy_stream;
	const int64_t nchunks = (npairs + chunk - 1) / chunk;
	auto dres = [&](int q, int a) { return (int32_t *)((char *)h->d_out + ((size_t)q * 4 + (size_t)a) * b_res); };
	auto hres = [&](int q, int a) { return (int32_t *)((char *)h->h_pin + ((size_t)q * 4 + (size_t)a) * b_res); };
	auto deliver = [&](int64_t c) -> int {
		const int q = (int)(c & 1);
		const int64_t lo = c * chunk, n = std::min(chunk, npairs - lo);
		HIP_TRY(h, hipEventSynchronize(h->ev_copy[q]));
		const int32_t *sc = hres(q, 0);
		for (int64_t p = 0; p < n; ++p)
			if (sc[p] == INT32_MIN)
				return fail(h, AT_ERR_DOMAIN, "pair %lld: input outside the domain on which the reference is defined", (long long)(first_pair + lo + p));
		if (fn && fn(user, first_pair + lo, n, sc, hres(q, 1), hres(q, 2), hres(q, 3)) != 0)
			return fail(h, AT_ERR_ARG, "all-vs-all: the caller's slice callback asked to stop at pair %lld", (long long)(first_pair + lo));
		return AT_OK;
	};
	std::string cfg0;
	for (int64_t c = 0; c < nchunks; ++c) {
		const int q = (int)(c & 1);
		const int64_t lo = c * chunk, n = std::min(chunk, npairs - lo);
		/* (slice c - 2, the last user of buffer set q, was delivered before slice c - 1 was queued) */
		BatchReq r = triangle_req(h, mode, rs, nreads, first_pair + lo, n, s);
		r.d_score = dres(q, 0); r.d_end_i = dres(q, 1); r.d_end_j = dres(q, 2); r.d_state = dres(q, 3);
		rc = align_device(h, r);
		if (rc) { (void)hipDeviceSynchronize(); return rc; }
		if (c == 0) cfg0 = h->cfg;
		HIP_TRY(h, hipEventRecord(h->ev_sweep[q], s));
		HIP_TRY(h, hipStreamWaitEvent(cs, h->ev_sweep[q], 0));
		for (int a = 0; a < 4; ++a) HIP_TRY(h, hipMemcpyAsync(hres(q, a), dres(q, a), (size_t)n * 4, hipMemcpyDeviceToHost, cs));
		HIP_TRY(h, hipEventRecord(h->ev_copy[q], cs));
		if (c >= 1) {
			rc = deliver(c - 1);
			if (rc) { (void)hipDeviceSynchronize(); return rc; }
		}
	}
	rc = deliver(nchunks - 1);
	if (rc) return rc;
	snprintf(h->cfg, sizeof h->cfg, "%.260s, %lld slices of <= %lld pairs", cfg0.c_str(), (long long)nchunks, (long long)chunk);
	return AT_OK;
}

extern "C" int at_align_allpairs_stream(at_handle *h, int mode, int64_t nreads, const uint8_t *seq_blob,
                                        const int64_t *off, const int32_t *len, int64_t first_pair, int64_t npairs,
                                        int64_t chunk_pairs, at_allpairs_chunk_fn fn, void *user)
{
	int rc = check_allpairs_args(h, "at_align_allpairs_stream", mode, nreads, first_pair, npairs);
	if (rc) return rc;
	if (npairs == 0) return AT_OK;
	if (!seq_blob || !off || !len || !fn) return fail(h, AT_ERR_ARG, "NULL argument");
	return guarded(h, "at_align_allpairs_stream", [&] {
		ReadSet rs;
		int rc2 = upload_reads(h, mode, nreads, seq_blob, off, len, &rs);
		if (rc2) return rc2;
		return allpairs_scores(h, mode, nreads, rs, first_pair, npairs, chunk_pairs, fn, user);
	});
}

/* ---- query-vs-target search: every query against every target, the best k hits of each query kept on the device ----
 * Queries and targets go up as ONE read set, queries first (one 2-bit / 8-bit decision for both, as all-vs-all).  The targets are
 * sorted by length (stable), the queries grouped by length: a BLOCK is one query-length group x the run of sorted targets it may
 * meet (fit: those no shorter than the query), cut into SLICES of at most AT_ALLPAIRS_CHUNK pairs.  Per slice, on the handle's stream
 * and without a host round trip: at_search_desc_k writes the slice's descriptors, align_device sweeps them (a block of one query
 * length x one target length with the uniform-shape promise: the packed kernels), at_search_merge_k folds the scores into the
 * per-query lists (at_search.hip).  The lists come down in one copy at the end. */
static const char *strands_text(int strands) { return strands == AT_STRAND_REV ? ", strands=rev" : strands == AT_STRAND_BOTH ? ", strands=both" : ""; }

/* ---- the scaffold of the query-vs-target entries (its host arithmetic: at_queryplan.h) ---- */
struct QuerySets {
	int64_t nq; const uint8_t *q_blob; const int64_t *q_off; const int32_t *q_len;
	int64_t nt; const uint8_t *t_blob; const int64_t *t_off; const int32_t *t_len;
};
struct ListOut { int32_t *target, *score, *end_i, *end_j, *state, *strand, *nhits; };
struct CigarOut {
	int32_t *stats, *ncigar; int64_t *off; uint32_t *words; int64_t cap;
	bool any() const { return stats || ncigar || off || words; }
};

/* the refusals the entries share, `who` naming the entry; each entry calls them in the order its checks always had */
static int check_sizes(at_handle *h, const char *who, int64_t nq, int64_t nt, int64_t cigar_cap, int k = 1)
{
	if (nq < 0 || nt < 0 || cigar_cap < 0) return fail(h, AT_ERR_ARG, "%s: negative size", who);
	if (k < 1 || k > 64) return fail(h, AT_ERR_ARG, "%s: k = %d outside 1..64", who, k);
	return AT_OK;
}

/* strands, tile width (0: the default, dflt_tile), flags, CIGAR outputs, read counts: no array is read */
static int check_options(at_handle *h, const char *who, int strands, int32_t tile_cols, int dflt_tile, int flags, const CigarOut &co, int64_t nq, int64_t nt)
{
	if (strands < AT_STRAND_FWD || strands > AT_STRAND_BOTH) return fail(h, AT_ERR_ARG, "%s: strands = %d outside 1..3", who, strands);
	if (tile_cols < 0 || (tile_cols & 15))
		return fail(h, AT_ERR_ARG, "%s: tile_cols = %d is not a positive multiple of 16 (or 0 for the default, %d)", who, tile_cols, dflt_tile);
	if (flags & ~AT_CIGAR_M) return fail(h, AT_ERR_ARG, "%s: flags = %d (AT_CIGAR_M or 0)", who, flags);
	if (co.any() && (!co.stats || !co.ncigar || !co.off || (!co.words && co.cap > 0)))
		return fail(h, AT_ERR_ARG, "%s: the CIGAR outputs are either all NULL or all given", who);
	if (nq + nt >= (1LL << 31)) return fail(h, AT_ERR_ARG, "%s: %lld queries + %lld targets: at most 2^31 - 1 reads", who, (long long)nq, (long long)nt);
	if (strands != AT_STRAND_FWD && (nt >= (1LL << 30) || 2 * nq + nt >= (1LL << 31)))
		return fail(h, AT_ERR_ARG, "%s: %lld queries, %lld targets: a reverse strand needs nt < 2^30 and 2 nq + nt < 2^31", who, (long long)nq, (long long)nt);
	return AT_OK;
}

static int check_one_gpu(at_handle *h, const char *who) { return h->comm ? fail(h, AT_ERR_DOMAIN, "%s: one GPU only (this handle belongs to a multi-process job)", who) : (int)AT_OK; }

static int check_list_pointers(at_handle *h, const char *who, const QuerySets &qt, const ListOut &o, bool rev)
{
	if (!qt.q_blob || !qt.q_off || !qt.q_len || !o.target || !o.score || !o.end_i || !o.end_j || !o.state || !o.nhits ||
	    (rev && !o.strand) || (qt.nt > 0 && (!qt.t_blob || !qt.t_off || !qt.t_len)))
		return fail(h, AT_ERR_ARG, "%s: NULL argument", who);
	return AT_OK;
}

static int check_read(at_handle *h, const char *what, int64_t i, int32_t len, int64_t off, bool need_base)
{
	if (len < 0 || off < 0) return fail(h, AT_ERR_ARG, "%s %lld: negative length or offset", what, (long long)i);
	if (need_base && len < 1) return fail(h, AT_ERR_DOMAIN, "%s %lld: empty", what, (long long)i);
	return AT_OK;
}

/* "no hit" in every list entry before any work */
static void list_out_init(const ListOut &o, int64_t nq, int k, const CigarOut &co)
{
	for (int64_t e = 0; e < nq * k; ++e) { o.target[e] = -1; o.score[e] = 0; o.end_i[e] = 0; o.end_j[e] = 0; o.state[e] = 0; }
	if (o.strand) for (int64_t e = 0; e < nq * k; ++e) o.strand[e] = -1;
	for (int64_t q = 0; q < nq; ++q) o.nhits[q] = 0;
	if (co.any()) {
		for (int64_t e = 0; e < nq * k; ++e) { co.ncigar[e] = 0; for (int x = 0; x < 8; ++x) co.stats[e * 8 + x] = -1; }
		for (int64_t e = 0; e <= nq * k; ++e) co.off[e] = 0;
	}
}

/* one read set: the queries' and the targets' bytes side by side (a copy of the input, small beside the sweep), queries first */
static int upload_sets(at_handle *h, int mode, const QuerySets &qt, bool rev, ReadSet *rs)
{
	const int64_t nq = qt.nq, nr = qt.nq + qt.nt;
	std::vector<int64_t> off((size_t)nr);
	std::vector<int32_t> len((size_t)nr);
	int64_t bytes = 0;
	for (int64_t r = 0; r < nr; ++r) { off[(size_t)r] = bytes; len[(size_t)r] = r < nq ? qt.q_len[r] : qt.t_len[r - nq]; bytes += len[(size_t)r]; }
	std::vector<uint8_t> blob((size_t)bytes + 32);
	for (int64_t r = 0; r < nr; ++r)
		if (len[(size_t)r]) memcpy(blob.data() + off[(size_t)r], r < nq ? qt.q_blob + qt.q_off[r] : qt.t_blob + qt.t_off[r - nq], (size_t)len[(size_t)r]);
	return upload_reads(h, mode, nr, blob.data(), off.data(), len.data(), rs, rev ? nq : 0);
}

/* the per-query lists in h->d_str: keys, end cells and states (20 bytes per entry), behind them the merges' `bad` word.  The lists
 * stay there behind the *_lists call: the window pass reads them */
struct ListBufs { unsigned long long *key; int *ei, *ej, *st, *bad; size_t bkey, bl4, lbytes; };
static int list_bufs(at_handle *h, size_t nl, bool with_bad, ListBufs *lb)
{
	return carve(h, &h->d_str, &h->str_bytes, [&](Carver &c) {
		lb->key = c.take<unsigned long long>(nl); lb->bkey = c.at;
		lb->ei = c.take<int>(nl); lb->bl4 = c.at - lb->bkey;
		lb->ej = c.take<int>(nl); lb->st = c.take<int>(nl);
		lb->bad = with_bad ? c.take<int>(1) : nullptr;
		lb->lbytes = c.at;
	});
}

/* the scores of the pairs [s0, s0 + n) of a block (entries from qa, ntb targets from ta) folded into the lists */
static int merge_slice(at_handle *h, const at::QueryOrder &qo, const ListBufs &lb, const int *d_qperm, const int *d_tperm, int32_t *const d_res[4],
                       int64_t s0, int64_t n, int64_t ntb, int qa, int ta, int k, int is_edit, int use_cutoff, int32_t cutoff)
{
	at::SearchMergeArgs ma;
	memset(&ma, 0, sizeof ma);
	ma.s0 = s0; ma.n = n; ma.ntb = ntb; ma.qa = qa; ma.ta = ta;
	ma.enc = qo.enc; ma.two = qo.two; ma.qperm = d_qperm; ma.tperm = d_tperm;
	ma.nqs = (int)((s0 + n - 1) / (ntb << qo.two) - s0 / (ntb << qo.two) + 1);
	ma.score = d_res[0]; ma.end_i = d_res[1]; ma.end_j = d_res[2]; ma.state = d_res[3];
	ma.k = k; ma.is_edit = is_edit; ma.use_cutoff = use_cutoff ? 1 : 0; ma.cutoff = cutoff;
	ma.lkey = lb.key; ma.lei = lb.ei; ma.lej = lb.ej; ma.lst = lb.st; ma.bad = lb.bad;
	HIP_TRY(h, at_search_merge_launch(&ma, h->stream));
	return AT_OK;
}

/* the lists come down in one copy, behind the call's one wait for its sweeps, and are decoded into the caller's arrays.  negate: the
 * ranks are negated distances; bad_who: the name under which a set `bad` word is an error, NULL: it is not looked at */
static int lists_readback(at_handle *h, const ListBufs &lb, int64_t nq, int k, int enc, bool negate, const char *bad_who, const ListOut &o)
{
	std::vector<char> hl(lb.lbytes);
	HIP_TRY(h, hipMemcpyAsync(hl.data(), lb.key, lb.lbytes, hipMemcpyDeviceToHost, h->stream));
	HIP_TRY(h, hipStreamSynchronize(h->stream));
	int bad = 0;
	memcpy(&bad, hl.data() + lb.bkey + 3 * lb.bl4, 4);
	if (bad && bad_who) return fail(h, AT_ERR_DOMAIN, "%s: a pair outside the domain on which the reference is defined", bad_who);
	const unsigned long long *hk = (const unsigned long long *)hl.data();
	const int32_t *hei = (const int32_t *)(hl.data() + lb.bkey), *hej = hei + lb.bl4 / 4, *hst = hej + lb.bl4 / 4;
	for (int64_t q = 0; q < nq; ++q) {
		int nh = 0;
		for (size_t e = (size_t)q * k; nh < k && hk[e]; ++e, ++nh) {
			const at::ListKey key = at::list_key_decode(hk[e], enc);
			o.target[e] = key.target;
			if (o.strand) o.strand[e] = key.strand;
			o.score[e] = negate ? -key.rank : key.rank;
			o.end_i[e] = hei[e]; o.end_j[e] = hej[e]; o.state[e] = hst[e];
		}
		o.nhits[q] = nh;
	}
	return AT_OK;
}

/* events on the handle's stream around a sweep phase: its device time goes into at_last_config (tools/edit_scan_rate.py and its kin) */
struct StreamEvents {
	hipEvent_t e[3] = {nullptr, nullptr, nullptr};
	~StreamEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
	int create(at_handle *h, int n) { for (int x = 0; x < n; ++x) HIP_TRY(h, hipEventCreate(&e[x])); return AT_OK; }
};

static int search_lists(at_handle *h, int mode, const QuerySets &qt, const ReadSet &rs, int k, int use_cutoff, int32_t cutoff, int strands,
                        const ListOut &out)
{
	const int64_t nq = qt.nq, nt = qt.nt;
	const int32_t *t_len = qt.t_len;
	const at::QueryOrder qo = at::query_order(nq, qt.q_len, strands);
	std::vector<int> tperm((size_t)nt);
	std::iota(tperm.begin(), tperm.end(), 0);
	std::stable_sort(tperm.begin(), tperm.end(), [&](int a, int b) { return t_len[a] < t_len[b]; });
	std::vector<int32_t> tls((size_t)nt);
	for (int64_t t = 0; t < nt; ++t) tls[(size_t)t] = t_len[tperm[(size_t)t]];
	struct Block { int qa, nqb, ta; int64_t ntb; int32_t l1, l2; bool uniform; };
	std::vector<Block> blocks;
	int64_t most = 0;
	for (const at::QueryBlock &Q : qo.blocks) {
		const int64_t ta = mode == AT_MODE_FIT ? std::lower_bound(tls.begin(), tls.end(), Q.l1) - tls.begin() : 0;
		if (ta == nt) continue;                                   /* fit: every target is shorter than these queries */
		blocks.push_back({Q.qa, Q.nqb, (int)ta, nt - ta, Q.l1, tls.back(), tls[(size_t)ta] == tls.back()});
		most = std::max<int64_t>(most, (int64_t)Q.nqb * (nt - ta));
	}
	const int64_t chunk = at::slice_clamp(env_ll("AT_ALLPAIRS_CHUNK", at::kSliceDefault), most);
	/* descriptors (24 bytes per pair of a slice) and both permutations; results (16 bytes per pair); the lists + flag */
	int64_t *d_woff1 = nullptr, *d_woff2 = nullptr; int32_t *d_len1 = nullptr, *d_len2 = nullptr, *d_r[4]; int *d_qperm = nullptr, *d_tperm = nullptr;
	ListBufs lb;
	int rc = carve(h, &h->d_desc, &h->desc_bytes, [&](Carver &c) {
		d_woff1 = c.take<int64_t>((size_t)chunk); d_woff2 = c.take<int64_t>((size_t)chunk);
		d_len1 = c.take<int32_t>((size_t)chunk); d_len2 = c.take<int32_t>((size_t)chunk);
		d_qperm = c.take<int>((size_t)qo.nv); d_tperm = c.take<int>((size_t)nt);
	});
	if (!rc) rc = carve(h, &h->d_out, &h->out_bytes, [&](Carver &c) { for (int32_t *&x : d_r) x = c.take<int32_t>((size_t)chunk); });
	if (!rc) rc = list_bufs(h, (size_t)nq * (size_t)k, true, &lb);
	if (rc) return rc;
	hipStream_t s = h->stream;
	HIP_TRY(h, hipMemcpyAsync(d_qperm, qo.qperm.data(), (size_t)qo.nv * 4, hipMemcpyHostToDevice, s));
	HIP_TRY(h, hipMemcpyAsync(d_tperm, tperm.data(), (size_t)nt * 4, hipMemcpyHostToDevice, s));
	HIP_TRY(h, hipMemsetAsync(lb.key, 0, lb.lbytes, s));
	std::string cfg0;
	int64_t nslices = 0;
	for (const Block &B : blocks) {
		const int64_t bp = (int64_t)B.nqb * B.ntb;
		for (int64_t s0 = 0; s0 < bp; s0 += chunk) {
			const int64_t n = std::min(chunk, bp - s0);
			at::SearchDescArgs da;
			memset(&da, 0, sizeof da);
			da.s0 = s0; da.n = n; da.ntb = B.ntb; da.qa = B.qa; da.ta = B.ta; da.nq = (int)nq; da.enc = qo.enc; da.nrev0 = (int)(nq + nt);
			da.qperm = d_qperm; da.tperm = d_tperm; da.swoff = (const long long *)rs.d_swoff; da.slen = rs.d_len;
			da.woff1 = (long long *)d_woff1; da.woff2 = (long long *)d_woff2; da.len1 = d_len1; da.len2 = d_len2;
			HIP_TRY(h, at_search_desc_launch(&da, h->ncu, s));
			BatchReq r(h);
			r.mode = mode; r.npairs = n; r.d_seq = rs.d_words; r.bits = rs.bits; r.stream = s;
			r.d_woff1 = d_woff1; r.d_len1 = d_len1; r.d_woff2 = d_woff2; r.d_len2 = d_len2; r.max_len1 = B.l1; r.max_len2 = B.l2;
			r.uniform_shape = B.uniform ? 1 : 0;
			r.d_score = d_r[0]; r.d_end_i = d_r[1]; r.d_end_j = d_r[2]; r.d_state = d_r[3];
			rc = align_device(h, r);
			if (rc) { (void)hipStreamSynchronize(s); return rc; }
			if (nslices == 0) cfg0 = h->cfg;
			rc = merge_slice(h, qo, lb, d_qperm, d_tperm, d_r, s0, n, B.ntb, B.qa, B.ta, k, mode == AT_MODE_EDIT, use_cutoff, cutoff);
			if (rc) return rc;
			++nslices;
		}
	}
	rc = lists_readback(h, lb, nq, k, qo.enc, mode == AT_MODE_EDIT, "search", out);
	if (rc) return rc;
	snprintf(h->cfg, sizeof h->cfg, "search: %lld blocks, %lld slices, k=%d%s; %.560s", (long long)blocks.size(), (long long)nslices, k,
	         strands_text(strands), cfg0.c_str());
	return AT_OK;
}

extern "C" int at_search_strands(at_handle *h, int mode,
                                 int64_t nq, const uint8_t *q_blob, const int64_t *q_off, const int32_t *q_len,
                                 int64_t nt, const uint8_t *t_blob, const int64_t *t_off, const int32_t *t_len,
                                 int k, int use_cutoff, int32_t cutoff, int strands,
                                 int32_t *out_target, int32_t *out_score, int32_t *out_end_i, int32_t *out_end_j,
                                 int32_t *out_state, int32_t *out_strand, int32_t *out_nhits)
{
	const char *who = "at_search";
	if (!h) return fail(nullptr, AT_ERR_ARG, "at_search: NULL handle");
	if (mode < AT_MODE_GLOBAL || mode > AT_MODE_EDIT) return fail(h, AT_ERR_ARG, "unknown mode %d", mode);
	const QuerySets qt = {nq, q_blob, q_off, q_len, nt, t_blob, t_off, t_len};
	const ListOut out = {out_target, out_score, out_end_i, out_end_j, out_state, out_strand, out_nhits};
	int rc = check_sizes(h, who, nq, nt, 0, k);
	if (rc || (rc = check_options(h, who, strands, 0, 0, 0, CigarOut{}, nq, nt))) return rc;
	const bool rev = strands != AT_STRAND_FWD;
	if (nq == 0) return AT_OK;
	if ((rc = check_list_pointers(h, who, qt, out, rev))) return rc;
	const bool need_base = mode == AT_MODE_LOCAL || mode == AT_MODE_OVERLAP;   /* (as upload_reads) */
	for (int64_t q = 0; q < nq; ++q) if ((rc = check_read(h, "query", q, q_len[q], q_off[q], need_base))) return rc;
	for (int64_t t = 0; t < nt; ++t) if ((rc = check_read(h, "target", t, t_len[t], t_off[t], need_base))) return rc;
	return guarded(h, who, [&]() -> int {
		list_out_init(out, nq, k, CigarOut{});
		if (nt == 0) { snprintf(h->cfg, sizeof h->cfg, "search: 0 blocks, 0 slices, k=%d%s; ", k, strands_text(strands)); return (int)AT_OK; }
		ReadSet rs;
		if (int rc2 = upload_sets(h, mode, qt, rev, &rs)) return rc2;
		return search_lists(h, mode, qt, rs, k, use_cutoff, cutoff, strands, out);
	});
}

extern "C" int at_search(at_handle *h, int mode,
                         int64_t nq, const uint8_t *q_blob, const int64_t *q_off, const int32_t *q_len,
                         int64_t nt, const uint8_t *t_blob, const int64_t *t_off, const int32_t *t_len,
                         int k, int use_cutoff, int32_t cutoff,
                         int32_t *out_target, int32_t *out_score, int32_t *out_end_i, int32_t *out_end_j,
                         int32_t *out_state, int32_t *out_nhits)
{
	return at_search_strands(h, mode, nq, q_blob, q_off, q_len, nt, t_blob, t_off, t_len, k, use_cutoff, cutoff, AT_STRAND_FWD,
	                         out_target, out_score, out_end_i, out_end_j, out_state, nullptr, out_nhits);
}

/* ---- reads against long targets (at_scan; at_scan.hip.h) ---- */
extern "C" int at_scan_plan(int32_t len1, int32_t len2, int use_cutoff, int32_t cutoff, int32_t tile_cols,
                            int32_t *tile, int32_t *overlap, int64_t *ngroups)
{
	at::ScanPlan sp;
	if (len1 < 0 || len2 < 0) return fail(nullptr, AT_ERR_ARG, "at_scan_plan: negative length");
	if (at::scan_plan(len1, len2, use_cutoff, cutoff, tile_cols, &sp) != AT_OK)
		return fail(nullptr, AT_ERR_ARG, "at_scan_plan: tile_cols = %d is not a positive multiple of 16 (or 0 for the default, %d)", tile_cols,
		            at::kScanDefaultTile);
	if (tile) *tile = sp.tile;
	if (overlap) *overlap = sp.overlap;
	if (ngroups) *ngroups = sp.ngroups;
	return AT_OK;
}

static const char *scan_strands_text(int strands) { return strands == AT_STRAND_REV ? "rev" : strands == AT_STRAND_BOTH ? "both" : "fwd"; }

/* what the sweeps of at_scan and at_scan_hits share: the targets' group prefix (gpre[t]: groups in front of target t, gall: of all), the
 * items in front of a pair, a block's kernel class and occupancy, a slice's arguments and grid, the first slice's words */
struct ScanSweep {
	int64_t nq, nt;
	int enc, tile, w, occ;   /* w, occ: of the block at hand */
	const ReadSet &rs;
	std::vector<long long> gpre;
	long long gall;
	ScanSweep(const QuerySets &qt, int enc_, int32_t tile_, const ReadSet &rs_) : nq(qt.nq), nt(qt.nt), enc(enc_), tile(tile_), w(0), occ(0), rs(rs_), gpre((size_t)qt.nt + 1, 0)
	{
		for (int64_t t = 0; t < nt; ++t) gpre[(size_t)t + 1] = gpre[(size_t)t] + at::scan_groups(qt.t_len[t], tile);
		gall = gpre[(size_t)nt];
	}
	long long items_before(int64_t x) const { return (long long)(x / nt) * gall + gpre[(size_t)(x % nt)]; }   /* items of the block's pairs [0, x) */
	int block(at_handle *h, int32_t l1, const void *(*kernel)(int))
	{
		w = at::class_rows(at::kMyersLaneWords, l1);
		const void *fn = kernel(w);
		if (!fn) return fail(h, AT_ERR_ARG, "no scan kernel for %d words per lane", w);
		occ = 0;
		if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, 64, 0) != hipSuccess || occ <= 0) occ = 8;
		return AT_OK;
	}
	at::ScanArgs slice(int qa, int64_t s0, int64_t n, const long long *d_gpre, const int *d_qperm, int use_cutoff, int32_t cutoff) const
	{
		at::ScanArgs sa;
		memset(&sa, 0, sizeof sa);
		sa.y0 = items_before(s0); sa.nitems = items_before(s0 + n) - sa.y0;
		sa.s0 = s0; sa.npairs = n; sa.ntb = nt; sa.gall = gall; sa.gpre = d_gpre;
		sa.qa = qa; sa.nq = (int)nq; sa.enc = enc; sa.nrev0 = (int)(nq + nt); sa.qperm = d_qperm;
		sa.seq = rs.d_words; sa.swoff = (const long long *)rs.d_swoff; sa.slen = rs.d_len;
		sa.tile = tile; sa.use_cutoff = use_cutoff ? 1 : 0; sa.cutoff = cutoff;
		return sa;
	}
	long long grid(const at_handle *h, const at::ScanArgs &sa) const { return std::max(1LL, std::min<long long>(sa.nitems, (long long)occ * h->ncu)); }
	std::string text(const char *kernel, long long grid) const
	{
		return std::string(kernel) + " bits=2 words/lane=" + std::to_string(w) + " (1 read/wave, 64 tiles) lds=0B waves/cu<=" + std::to_string(occ) + " grid=" + std::to_string(grid);
	}
};

/* the lists of at_scan: the blocks and slices of search_lists with the targets in caller order; per slice the key slots are set,
 * the groups of its pairs swept, the keys unpacked and merged (at_scan.hip.h).  (The merges' `bad` word is not looked at.) */
static int scan_lists(at_handle *h, const QuerySets &qt, const ReadSet &rs, int k, int use_cutoff, int32_t cutoff, int strands, int32_t tile,
                      const ListOut &out, ListBufs &lb)
{
	const int64_t nq = qt.nq, nt = qt.nt;
	const at::QueryOrder qo = at::query_order(nq, qt.q_len, strands);
	std::vector<int> tperm((size_t)nt);   /* (the targets stay in caller order) */
	std::iota(tperm.begin(), tperm.end(), 0);
	ScanSweep sw(qt, qo.enc, tile, rs);
	int64_t most = 0;
	for (const at::QueryBlock &B : qo.blocks) most = std::max<int64_t>(most, (int64_t)B.nqb * nt);
	const int64_t chunk = at::slice_clamp(env_ll("AT_ALLPAIRS_CHUNK", at::kSliceDefault), most);
	unsigned long long *d_pkey = nullptr; long long *d_gpre = nullptr; int *d_qperm = nullptr, *d_tperm = nullptr; int32_t *d_r[4];
	int rc = carve(h, &h->d_desc, &h->desc_bytes, [&](Carver &c) {
		d_pkey = c.take<unsigned long long>((size_t)chunk); d_gpre = c.take<long long>((size_t)nt + 1);
		d_qperm = c.take<int>((size_t)qo.nv); d_tperm = c.take<int>((size_t)nt);
	});
	if (!rc) rc = carve(h, &h->d_out, &h->out_bytes, [&](Carver &c) { for (int32_t *&x : d_r) x = c.take<int32_t>((size_t)chunk); });
	if (!rc) rc = list_bufs(h, (size_t)nq * (size_t)k, true, &lb);
	if (rc) return rc;
	hipStream_t s = h->stream;
	HIP_TRY(h, hipMemcpyAsync(d_qperm, qo.qperm.data(), (size_t)qo.nv * 4, hipMemcpyHostToDevice, s));
	HIP_TRY(h, hipMemcpyAsync(d_tperm, tperm.data(), (size_t)nt * 4, hipMemcpyHostToDevice, s));
	HIP_TRY(h, hipMemcpyAsync(d_gpre, sw.gpre.data(), ((size_t)nt + 1) * 8, hipMemcpyHostToDevice, s));
	HIP_TRY(h, hipMemsetAsync(lb.key, 0, lb.lbytes, s));
	std::string cfg0;
	int64_t nslices = 0, ov_most = 0;
	StreamEvents ev;   /* (around key slots, groups, unpack and merge of every slice) */
	if ((rc = ev.create(h, 2))) return rc;
	HIP_TRY(h, hipEventRecord(ev.e[0], s));
	for (const at::QueryBlock &B : qo.blocks) {
		const int64_t bp = (int64_t)B.nqb * nt;
		if ((rc = sw.block(h, B.l1, at_scan_kernel))) return rc;
		ov_most = std::max<int64_t>(ov_most, at::scan_overlap(B.l1, use_cutoff, cutoff));
		for (int64_t s0 = 0; s0 < bp; s0 += chunk) {
			const int64_t n = std::min(chunk, bp - s0);
			at::ScanArgs sa = sw.slice(B.qa, s0, n, d_gpre, d_qperm, use_cutoff, cutoff);
			sa.key = d_pkey; sa.score = d_r[0]; sa.end_i = d_r[1]; sa.end_j = d_r[2]; sa.state = d_r[3];
			HIP_TRY(h, at_scan_init_launch(&sa, h->ncu, s));
			if (int rcq = ensure_queue(h, s)) return rcq;
			sa.queue = h->d_queue;
			const long long grid = sw.grid(h, sa);
			HIP_TRY(h, at_scan_launch(&sa, sw.w, (unsigned)grid, s));
			HIP_TRY(h, at_scan_unpack_launch(&sa, h->ncu, s));
			if (nslices == 0) cfg0 = sw.text("myers-scan", grid);
			if ((rc = merge_slice(h, qo, lb, d_qperm, d_tperm, d_r, s0, n, nt, B.qa, 0, k, 1, use_cutoff, cutoff))) return rc;
			++nslices;
		}
	}
	HIP_TRY(h, hipEventRecord(ev.e[1], s));
	if ((rc = lists_readback(h, lb, nq, k, qo.enc, true, nullptr, out))) return rc;
	float sweep_ms = 0.f;
	HIP_TRY(h, hipEventElapsedTime(&sweep_ms, ev.e[0], ev.e[1]));
	snprintf(h->cfg, sizeof h->cfg, "scan: tile=%d overlap<=%d groups=%lld k=%d strands=%s, %lld blocks, %lld slices; %s sweep=%.3fms", tile, (int)ov_most, sw.gall, k,
	         scan_strands_text(strands), (long long)qo.blocks.size(), (long long)nslices, cfg0.c_str(), (double)sweep_ms);
	return AT_OK;
}

/* what the window passes (the alignments of hits) share.  window_carve: the device arrays, in h->d_out [front bytes |] three 64-bit arrays
 * [| the hits' list entries] | eight 32-bit arrays, in h->d_cg the run counts [| a second set] | statistics | word offsets | the words for
 * dcap | `bad`, and the op slots in a buffer the family names.  window_fetch: counts, statistics and offsets into the caller's arrays
 * behind the pass's one wait; a set `bad` word is bad_text.  window_words: the words that end within the caller's room */
struct WindowBufs {
	void *front; int64_t *woff1, *woff2, *ops_off, *coff; long long *eidx; uint32_t *cigar; int *bad; uint8_t *ops;
	int32_t *len1, *len2, *aux, *sc, *ei, *ej, *st, *nops, *ncigar, *ncout, *stats;   /* aux: the windows' starts, or the pairs' slot sizes */
};

/* the traceback pass over n windows: their descriptors, results and op slots */
static BatchReq window_req(const at_handle *h, int mode, int64_t n, const ReadSet &rs, const WindowBufs &w, int32_t max1, int32_t max2, hipStream_t s)
{
	BatchReq r(h);
	r.mode = mode; r.npairs = n; r.d_seq = rs.d_words; r.bits = rs.bits; r.stream = s;
	r.d_woff1 = w.woff1; r.d_len1 = w.len1; r.d_woff2 = w.woff2; r.d_len2 = w.len2; r.max_len1 = max1; r.max_len2 = max2;
	r.want_traceback = 1;
	r.d_score = w.sc; r.d_end_i = w.ei; r.d_end_j = w.ej; r.d_state = w.st;
	r.d_ops = w.ops; r.d_ops_off = w.ops_off; r.d_nops = w.nops;
	return r;
}

static int window_carve(at_handle *h, int64_t n, int64_t dcap, size_t front_bytes, bool eidx, bool ncout, void **ops_buf, size_t *ops_have, size_t ops_need,
                        WindowBufs &w)
{
	int rc = carve(h, &h->d_out, &h->out_bytes, [&](Carver &c) {
		w.front = c.take<char>(front_bytes);
		w.woff1 = c.take<int64_t>((size_t)n + 1); w.woff2 = c.take<int64_t>((size_t)n + 1); w.ops_off = c.take<int64_t>((size_t)n + 1);
		w.eidx = eidx ? c.take<long long>((size_t)n + 1) : nullptr;
		for (int32_t **x : {&w.len1, &w.len2, &w.aux, &w.sc, &w.ei, &w.ej, &w.st, &w.nops}) *x = c.take<int32_t>((size_t)n);
	});
	if (!rc) rc = grow(h, ops_buf, ops_have, ops_need);
	if (!rc) rc = carve(h, &h->d_cg, &h->cg_bytes, [&](Carver &c) {
		w.ncigar = c.take<int32_t>((size_t)n);
		w.ncout = ncout ? c.take<int32_t>((size_t)n) : w.ncigar;
		w.stats = c.take<int32_t>((size_t)n * 8); w.coff = c.take<int64_t>((size_t)n + 1);
		w.cigar = c.take<uint32_t>((size_t)dcap); w.bad = c.take<int>(1);
	});
	w.ops = (uint8_t *)*ops_buf;
	return rc;
}

static int window_fetch(at_handle *h, const WindowBufs &w, int64_t n, const char *bad_text, int32_t *out_ncigar, int32_t *out_stats, int64_t *out_off)
{
	int bad = 0;
	hipStream_t s = h->stream;
	HIP_TRY(h, hipMemcpyAsync(&bad, w.bad, 4, hipMemcpyDeviceToHost, s));
	HIP_TRY(h, hipMemcpyAsync(out_ncigar, w.ncout, (size_t)n * 4, hipMemcpyDeviceToHost, s));
	HIP_TRY(h, hipMemcpyAsync(out_stats, w.stats, (size_t)n * 32, hipMemcpyDeviceToHost, s));
	HIP_TRY(h, hipMemcpyAsync(out_off, w.coff, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, s));
	HIP_TRY(h, hipStreamSynchronize(s));
	return bad ? fail(h, AT_ERR_RANGE, "%s", bad_text) : (int)AT_OK;
}

static int window_words(at_handle *h, const WindowBufs &w, const int64_t *off, int64_t n, int64_t room, uint32_t *out_cigar)
{
	const int64_t fit = at::prefix_fit(off, n, room);
	if (fit > 0) {
		HIP_TRY(h, hipMemcpyAsync(out_cigar, w.cigar, (size_t)fit * 4, hipMemcpyDeviceToHost, h->stream));
		HIP_TRY(h, hipStreamSynchronize(h->stream));
	}
	return AT_OK;
}

/* the alignments of the hits: every list entry as a window pair through at_infix<W, true> and the CIGAR kernels (at_scan.hip.h) */
/* at_scan: the n = nq * k list entries, entry e of query e / k, windows that end in their arg-min.  at_scan_hits (who names the caller
 * in an error text): n hits with their queries in lb.ei and END-ANCHORED windows -- a hit that is not the best of its triple is not the
 * arg-min of its window */
static int scan_cigars(at_handle *h, int64_t nq, int k, int strands, const ReadSet &rs, int64_t nt, int32_t maxq, const ListBufs &lb,
                       const int32_t *out_target, const int32_t *out_score, const int32_t *out_end_i, const int32_t *out_end_j, int flags,
                       const CigarOut &co, int64_t nhits = -1, const char *who = "at_scan")
{
	const int64_t n = nhits >= 0 ? nhits : nq * k;
	const int anchor = nhits >= 0 ? 1 : 0;
	/* ops slots: l1 + window columns per hit, back to back */
	std::vector<int64_t> slot((size_t)n);
	int64_t ops_bytes = 0;
	int32_t max2 = 0;
	for (int64_t e = 0; e < n; ++e) {
		slot[(size_t)e] = ops_bytes;
		if (out_target[e] < 0) continue;
		const int32_t len2 = (int32_t)(out_end_j[e] - at::scan_window_start(out_end_j[e], out_end_i[e], out_score[e]));
		ops_bytes += (int64_t)out_end_i[e] + len2;
		max2 = std::max(max2, len2);
	}
	const int64_t dcap = std::min<int64_t>(co.cap, ops_bytes);   /* (a list has no more runs than ops) */
	char bad_text[256];
	snprintf(bad_text, sizeof bad_text, "%s: a hit's window does not reproduce its score and end column (target columns [ws, j*) of at most %d)", who, max2);
	hipStream_t s = h->stream;
	WindowBufs w;
	int rc = window_carve(h, n, dcap, 0, false, true, &h->d_order, &h->order_bytes, (size_t)ops_bytes + 256, w);
	if (rc) return rc;
	HIP_TRY(h, hipMemcpyAsync(w.ops_off, slot.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
	HIP_TRY(h, hipMemsetAsync(w.bad, 0, 4, s));
	at::ScanWindowArgs wa;
	memset(&wa, 0, sizeof wa);
	wa.n = n; wa.k = k; wa.nq = (int)nq; wa.enc = strands != AT_STRAND_FWD; wa.nrev0 = (int)(nq + nt);
	wa.lkey = lb.key; wa.lej = lb.ej; wa.eq = anchor ? lb.ei : nullptr;
	wa.swoff = (const long long *)rs.d_swoff; wa.slen = rs.d_len;
	wa.woff1 = (long long *)w.woff1; wa.woff2 = (long long *)w.woff2; wa.len1 = w.len1; wa.len2 = w.len2; wa.ws = w.aux;
	wa.w_score = w.sc; wa.w_end_j = w.ej; wa.ncigar = w.ncigar; wa.stats = w.stats; wa.ncigar_out = w.ncout; wa.bad = w.bad;
	HIP_TRY(h, at_scan_window_launch(&wa, h->ncu, s));
	const std::string cfg0 = h->cfg;
	/* the window pass is an infix batch with op lists whatever the handle's settings say */
	BatchReq r = window_req(h, AT_MODE_EDIT, n, rs, w, maxq, max2, s);
	r.bits = 2;
	r.edit_infix = 1; r.edit_tb = 1; r.infix_anchor = anchor;
	rc = align_device(h, r);
	if (rc) { (void)hipStreamSynchronize(s); return rc; }
	const std::string cfg1 = h->cfg;
	rc = at_cigar_batch_device(h, n, rs.d_words, 2, w.woff1, w.woff2, w.ei, w.ej, w.ops, w.ops_off, w.nops, flags, w.ncigar, w.stats, w.coff, w.cigar, dcap, s);
	if (rc) { (void)hipStreamSynchronize(s); return rc; }
	HIP_TRY(h, at_scan_check_launch(&wa, h->ncu, s));
	if ((rc = window_fetch(h, w, n, bad_text, co.ncigar, co.stats, co.off)) || (rc = window_words(h, w, co.off, n, co.cap, co.words))) return rc;
	snprintf(h->cfg, sizeof h->cfg, "%.300s; windows: %.200s, cigars: %d lanes/pair", cfg0.c_str(), cfg1.c_str(), h->last_cigar_lanes);
	return AT_OK;
}

extern "C" int at_scan(at_handle *h,
                       int64_t nq, const uint8_t *q_blob, const int64_t *q_off, const int32_t *q_len,
                       int64_t nt, const uint8_t *t_blob, const int64_t *t_off, const int32_t *t_len,
                       int k, int use_cutoff, int32_t cutoff, int strands, int32_t tile_cols, int flags,
                       int32_t *out_target, int32_t *out_score, int32_t *out_end_i, int32_t *out_end_j,
                       int32_t *out_state, int32_t *out_strand, int32_t *out_nhits,
                       int32_t *out_stats, int32_t *out_ncigar, int64_t *out_cigar_off,
                       uint32_t *out_cigar, int64_t cigar_cap)
{
	const char *who = "at_scan";
	if (!h) return fail(nullptr, AT_ERR_ARG, "at_scan: NULL handle");
	const QuerySets qt = {nq, q_blob, q_off, q_len, nt, t_blob, t_off, t_len};
	const ListOut out = {out_target, out_score, out_end_i, out_end_j, out_state, out_strand, out_nhits};
	const CigarOut co = {out_stats, out_ncigar, out_cigar_off, out_cigar, cigar_cap};
	int rc = check_sizes(h, who, nq, nt, cigar_cap, k);
	if (rc || (rc = check_options(h, who, strands, tile_cols, at::kScanDefaultTile, flags, co, nq, nt)) || (rc = check_one_gpu(h, who))) return rc;
	const bool rev = strands != AT_STRAND_FWD;
	if (h->u != 1) return fail(h, AT_ERR_DOMAIN, "at_scan needs the unit mismatch cost: u = %d, not 1", h->u);
	if (nq == 0) return AT_OK;
	if ((rc = check_list_pointers(h, who, qt, out, rev))) return rc;
	int32_t maxq = 0;
	for (int64_t q = 0; q < nq; ++q) {
		if ((rc = check_read(h, "query", q, q_len[q], q_off[q], false))) return rc;
		if (q_len[q] > at::kScanMaxQuery) return fail(h, AT_ERR_DOMAIN, "at_scan: query %lld has %d bases, more than %d", (long long)q, q_len[q], at::kScanMaxQuery);
		maxq = std::max(maxq, q_len[q]);
	}
	for (int64_t t = 0; t < nt; ++t) if ((rc = check_read(h, "target", t, t_len[t], t_off[t], false))) return rc;
	const int32_t tile = tile_cols > 0 ? tile_cols : at::kScanDefaultTile;
	return guarded(h, who, [&]() -> int {
		list_out_init(out, nq, k, co);
		if (nt == 0) {
			snprintf(h->cfg, sizeof h->cfg, "scan: tile=%d overlap<=0 groups=0 k=%d strands=%s, 0 blocks, 0 slices; ", tile, k, scan_strands_text(strands));
			return (int)AT_OK;
		}
		ReadSet rs;
		int rc2 = upload_sets(h, AT_MODE_EDIT, qt, rev, &rs);
		if (rc2) return rc2;
		if (rs.bits != 2) return fail(h, AT_ERR_DOMAIN, "at_scan needs 2-bit reads: some base of a query or a target is not one of ACGT");
		ListBufs lb;
		if ((rc2 = scan_lists(h, qt, rs, k, use_cutoff, cutoff, strands, tile, out, lb)) || !co.any()) return rc2;
		return scan_cigars(h, nq, k, strands, rs, nt, maxq, lb, out_target, out_score, out_end_i, out_end_j, flags, co);
	});
}

/* ---- reads against long targets, cut into tiles: Smith-Waterman (at_scan_local) and end-to-end affine alignment
 * (at_scan_fit, 3.18); at_tilescan.hip.h ---- */
/* what the two scans do differently on the host (the kernels' side: at_tilescan.hip.h); their texts, which differ in the order of
 * their fields, stand as literals where they are written, local's beside fit's */
struct TileScanFamily {
	const char *who;                 /* the entry's name */
	int mode;                        /* AT_MODE_LOCAL / AT_MODE_FIT: the sweep of a tile and of a window, the family of the kernels */
	int32_t default_tile;
	bool by_length;                  /* the targets sorted by length, a block's targets those no shorter than its queries (search_lists) */
	bool target_need_base;           /* an empty target is an error (fit: it is shorter than every query: no candidate, no error) */
	int64_t (*overlap)(int32_t l1, int use_cutoff, int32_t cutoff, int m, int u, int o, int e);
	int (*check_scoring)(at_handle *h);                          /* the entry's refusals of a scoring, in its order */
	int (*check_query)(at_handle *h, int64_t q, int32_t len);
	/* a tile is a pair of the batch entry: its exact-score bound (align_device), said with the tile's numbers */
	int (*check_range)(at_handle *h, int32_t l1, int32_t tile, int64_t ov, int32_t maxt, long long maxabs);
	int32_t (*window_len)(const at_handle *h, int32_t l1, int32_t l2, int32_t score, int32_t end_i, int32_t end_j);   /* target columns of a hit's window */
};

static const TileScanFamily kScanLocal = {
	"at_scan_local", AT_MODE_LOCAL, at::kLocalScanDefaultTile, false, true,
	at::localscan_overlap,
	[](at_handle *h) -> int {
		if (at::localscan_scoring_ok(h->m, h->o, h->e) != AT_OK)
			return fail(h, AT_ERR_DOMAIN, "at_scan_local needs m >= 1, o <= -1 and e <= -1: m = %d, o = %d, e = %d", h->m, h->o, h->e);
		return AT_OK;
	},
	[](at_handle *h, int64_t q, int32_t len) -> int {
		if (at::localscan_query_ok(len, h->m, h->u) != AT_OK)
			return fail(h, AT_ERR_DOMAIN, "at_scan_local: query %lld has %d bases: at most %d, and max(m, u) * length < 2^%d", (long long)q, len,
			            at::kLocalScanMaxQuery, at::kLocalScanScoreBits);
		return AT_OK;
	},
	[](at_handle *h, int32_t l1, int32_t tile, int64_t ov, int32_t, long long maxabs) -> int {
		if (maxabs * ((long long)l1 + tile + ov + 2) >= (1LL << 24))
			return fail(h, AT_ERR_RANGE, "at_scan_local: a tile of %d rows x %d + %lld columns may leave the exact score range: max|param| = %lld", l1,
			            tile, (long long)ov, maxabs);
		return AT_OK;
	},
	[](const at_handle *h, int32_t, int32_t, int32_t score, int32_t end_i, int32_t end_j) -> int32_t {
		return (int32_t)(end_j - at::localscan_window_start(end_j, end_i, score, h->m, h->u, h->o, h->e));
	},
};

static const TileScanFamily kScanFit = {
	"at_scan_fit", AT_MODE_FIT, at::kFitScanDefaultTile, true, false,
	at::fitscan_overlap,
	[](at_handle *h) -> int {
		if (at::fitscan_scoring_ok(h->m, h->o, h->e) != AT_OK)
			return fail(h, AT_ERR_DOMAIN, "at_scan_fit needs m >= 1, o <= -1 and e <= -1: m = %d, o = %d, e = %d", h->m, h->o, h->e);
		if (h->use_jump) return fail(h, AT_ERR_DOMAIN, "at_scan_fit: jump sites (fit -s) are per-target columns and are not scanned: use_jump is set");
		return AT_OK;
	},
	[](at_handle *h, int64_t q, int32_t len) -> int {
		if (at::fitscan_query_ok(len) != AT_OK)
			return fail(h, AT_ERR_DOMAIN, "at_scan_fit: query %lld has %d bases: at most %d", (long long)q, len, at::kFitScanMaxQuery);
		return AT_OK;
	},
	[](at_handle *h, int32_t l1, int32_t tile, int64_t ov, int32_t maxt, long long maxabs) -> int {
		const int64_t full_len = std::min<int64_t>(maxt, tile + ov);   /* the longest tile of the block */
		if (maxabs * ((long long)l1 + full_len + 2) >= (1LL << 24))
			return fail(h, AT_ERR_RANGE, "at_scan_fit: a tile of %d rows x %lld columns (tile = %d, overlap = %lld) may leave the exact score range: max|param| = %lld",
			            l1, (long long)full_len, tile, (long long)ov, maxabs);
		return AT_OK;
	},
	[](const at_handle *h, int32_t l1, int32_t l2, int32_t score, int32_t, int32_t end_j) -> int32_t {
		const int64_t ws = at::fitscan_window_start(end_j, l1, score, h->m, h->u, h->o, h->e);
		return (int32_t)(at::fitscan_window_end(end_j, ws, l1, l2) - ws);
	},
};

/* what at_scan_local_plan and at_scan_fit_plan make of their planner's answer */
template <typename Plan>
static int tilescan_plan_out(const TileScanFamily &F, int rc, const Plan &sp, int32_t tile_cols, int32_t *tile, int32_t *overlap, int64_t *ntiles, int64_t *nfull)
{
	if (rc == AT_ERR_ARG)
		return fail(nullptr, AT_ERR_ARG, "%s_plan: a negative length, or tile_cols = %d is not a positive multiple of 16 (or 0 for the default, %d)", F.who,
		            tile_cols, F.default_tile);
	if (rc != AT_OK) {
		if (F.mode == AT_MODE_FIT)
			return fail(nullptr, AT_ERR_DOMAIN, "at_scan_fit_plan: needs m >= 1, o <= -1, e <= -1, a query of 1 .. %d bases and a tile + overlap below 2^31",
			            at::kFitScanMaxQuery);
		else
			return fail(nullptr, AT_ERR_DOMAIN, "at_scan_local_plan: needs m >= 1, o <= -1, e <= -1 and a query of 1 .. %d bases with max(m, u) * length < 2^%d",
			            at::kLocalScanMaxQuery, at::kLocalScanScoreBits);
	}
	if (tile) *tile = sp.tile;
	if (overlap) *overlap = sp.overlap;
	if (ntiles) *ntiles = sp.ntiles;
	if (nfull) *nfull = sp.nfull;
	return AT_OK;
}

extern "C" int at_scan_local_plan(int32_t len1, int32_t len2, int use_cutoff, int32_t cutoff, int32_t tile_cols, int m, int u, int o, int e,
                                  int32_t *tile, int32_t *overlap, int64_t *ntiles, int64_t *nfull)
{
	at::LocalScanPlan sp;
	const int rc = at::localscan_plan(len1, len2, use_cutoff, cutoff, tile_cols, m, u, o, e, &sp);
	return tilescan_plan_out(kScanLocal, rc, sp, tile_cols, tile, overlap, ntiles, nfull);
}

extern "C" int at_scan_fit_plan(int32_t len1, int32_t len2, int use_cutoff, int32_t cutoff, int32_t tile_cols, int m, int u, int o, int e,
                                int32_t *tile, int32_t *overlap, int64_t *ntiles, int64_t *nfull)
{
	at::FitScanPlan sp;
	const int rc = at::fitscan_plan(len1, len2, use_cutoff, cutoff, tile_cols, m, u, o, e, &sp);
	return tilescan_plan_out(kScanFit, rc, sp, tile_cols, tile, overlap, ntiles, nfull);
}

extern "C" int64_t at_scan_local_window(int32_t end_i, int64_t end_j, int32_t score, int m, int u, int o, int e)
{
	if (o == 0 || e == 0) return 0;
	return at::localscan_window_start(end_j, end_i, score, m, u, o, e);
}

extern "C" int at_scan_fit_window(int64_t end_j, int32_t score, int32_t len1, int32_t len2, int m, int u, int o, int e, int64_t *ws, int64_t *we)
{
	if (at::fitscan_scoring_ok(m, o, e) != AT_OK || at::fitscan_query_ok(len1) != AT_OK)
		return fail(nullptr, AT_ERR_DOMAIN, "at_scan_fit_window: needs m >= 1, o <= -1, e <= -1 and a query of 1 .. %d bases", at::kFitScanMaxQuery);
	if (len2 < len1 || end_j < 0 || end_j >= len2)
		return fail(nullptr, AT_ERR_ARG, "at_scan_fit_window: no hit of a %d x %d pair ends in column %lld", len1, len2, (long long)end_j);
	const int64_t s = at::fitscan_window_start(end_j, len1, score, m, u, o, e);
	if (ws) *ws = s;
	if (we) *we = at::fitscan_window_end(end_j, s, len1, len2);
	return AT_OK;
}

/* the lists of a tiled scan: the blocks of search_lists, for local with the targets in caller order and every block against all of
 * them, for fit with the targets sorted by length and a block's targets those no shorter than its queries.  A block's pairs go in
 * RUNS of at most `chunk` pairs whose key slots stay until every tile of the run is folded; a run's tiles go in two passes (the
 * tiles of the full shape, a uniform batch, and the shorter ones at the targets' ends) and each pass in SLICES of at most `chunk`
 * tile pairs: descriptors, the batch entry's sweep, fold.  Behind the last slice the run's slots are unpacked and merged.  The lists
 * stay in h->d_str behind the call. */
static int tilescan_lists(at_handle *h, const TileScanFamily &F, const QuerySets &qt, const ReadSet &rs, int k, int use_cutoff, int32_t cutoff, int strands,
                          int32_t tile, const ListOut &out, ListBufs &lb)
{
	const int64_t nq = qt.nq, nt = qt.nt;
	const int32_t *t_len = qt.t_len;
	const at::QueryOrder qo = at::query_order(nq, qt.q_len, strands);
	std::vector<int> tperm((size_t)nt);
	std::iota(tperm.begin(), tperm.end(), 0);
	if (F.by_length) std::stable_sort(tperm.begin(), tperm.end(), [&](int a, int b) { return t_len[a] < t_len[b]; });
	std::vector<int32_t> tls((size_t)nt);
	for (int64_t t = 0; t < nt; ++t) tls[(size_t)t] = t_len[tperm[(size_t)t]];
	struct Block { int qa, nqb, ta; int64_t ntb; int32_t l1; };
	std::vector<Block> blocks;
	int64_t most = 0;
	for (const at::QueryBlock &Q : qo.blocks) {
		const int64_t ta = F.by_length ? std::lower_bound(tls.begin(), tls.end(), Q.l1) - tls.begin() : 0;
		if (ta == nt) continue;                                   /* every target is shorter than these queries */
		blocks.push_back({Q.qa, Q.nqb, (int)ta, nt - ta, Q.l1});
		most = std::max<int64_t>(most, (int64_t)Q.nqb * (nt - ta));
	}
	const int32_t maxt = *std::max_element(tls.begin(), tls.end());
	/* a slice holds tile pairs: a run has at least as many tiles as pairs; its bound is that of the largest block's tiles (an upper bound:
	 * some are not swept) */
	const int64_t chunk = at::slice_clamp(env_ll("AT_ALLPAIRS_CHUNK", at::kSliceDefault), most * std::max<int64_t>(1, at::localscan_tiles(maxt, tile)));
	int64_t *d_woff1 = nullptr, *d_woff2 = nullptr; long long *d_s0 = nullptr, *d_slot = nullptr, *d_tpre[2]; unsigned long long *d_pkey = nullptr;
	int32_t *d_len1 = nullptr, *d_len2 = nullptr, *d_r[8]; int *d_qperm = nullptr, *d_tperm = nullptr;
	int rc = carve(h, &h->d_desc, &h->desc_bytes, [&](Carver &c) {
		d_woff1 = c.take<int64_t>((size_t)chunk); d_woff2 = c.take<int64_t>((size_t)chunk);
		d_s0 = c.take<long long>((size_t)chunk); d_slot = c.take<long long>((size_t)chunk);
		d_pkey = c.take<unsigned long long>((size_t)chunk);
		d_len1 = c.take<int32_t>((size_t)chunk); d_len2 = c.take<int32_t>((size_t)chunk);
		for (long long *&x : d_tpre) x = c.take<long long>((size_t)nt + 1);
		d_qperm = c.take<int>((size_t)qo.nv); d_tperm = c.take<int>((size_t)nt);
	});
	if (!rc) rc = carve(h, &h->d_out, &h->out_bytes, [&](Carver &c) { for (int32_t *&x : d_r) x = c.take<int32_t>((size_t)chunk); });
	if (!rc) rc = list_bufs(h, (size_t)nq * (size_t)k, true, &lb);
	if (rc) return rc;
	hipStream_t s = h->stream;
	HIP_TRY(h, hipMemcpyAsync(d_qperm, qo.qperm.data(), (size_t)qo.nv * 4, hipMemcpyHostToDevice, s));
	HIP_TRY(h, hipMemcpyAsync(d_tperm, tperm.data(), (size_t)nt * 4, hipMemcpyHostToDevice, s));
	HIP_TRY(h, hipMemsetAsync(lb.key, 0, lb.lbytes, s));
	std::string cfg0;
	int64_t nslices = 0, tiles_all = 0, ov_most = 0;
	StreamEvents ev;
	if ((rc = ev.create(h, 2))) return rc;
	HIP_TRY(h, hipEventRecord(ev.e[0], s));
	long long maxabs = 1;
	for (int v : {h->m, h->u, h->o, h->e, h->j}) maxabs = std::max<long long>(maxabs, std::llabs((long long)v));
	std::vector<long long> tpre[2];
	for (const Block &B : blocks) {
		/* the overlap depends on the query length: the block's prefix arrays of full and of shorter tiles per target */
		const int64_t ov = F.overlap(B.l1, use_cutoff, cutoff, h->m, h->u, h->o, h->e);
		if ((rc = F.check_range(h, B.l1, tile, ov, maxt, maxabs))) return rc;
		ov_most = std::max(ov_most, ov);
		const at::BlockTiles bt = at::block_tiles(tls.data() + B.ta, B.ntb, tile, ov, tpre);
		tiles_all += bt.tiles * B.nqb;
		/* (the copies read the vectors when they run: the stream is drained before the next block rewrites them) */
		for (int x = 0; x < 2; ++x) HIP_TRY(h, hipMemcpyAsync(d_tpre[x], tpre[x].data(), ((size_t)B.ntb + 1) * 8, hipMemcpyHostToDevice, s));
		HIP_TRY(h, hipStreamSynchronize(s));
		const int64_t bp = (int64_t)B.nqb * B.ntb;
		for (int64_t p0 = 0; p0 < bp; p0 += chunk) {
			const int64_t n = std::min(chunk, bp - p0);
			at::TileScanArgs sa;
			memset(&sa, 0, sizeof sa);
			sa.cap = chunk; sa.p0 = p0; sa.npairs = n; sa.ntb = B.ntb;
			sa.qa = B.qa; sa.ta = B.ta; sa.nq = (int)nq; sa.enc = qo.enc; sa.nrev0 = (int)(nq + nt); sa.bpw = rs.bits == 2 ? 16 : 4;
			sa.qperm = d_qperm; sa.tperm = d_tperm;
			sa.swoff = (const long long *)rs.d_swoff; sa.slen = rs.d_len; sa.tile = tile; sa.overlap = ov;
			sa.woff1 = (long long *)d_woff1; sa.woff2 = (long long *)d_woff2; sa.len1 = d_len1; sa.len2 = d_len2; sa.s0 = d_s0; sa.slot = d_slot;
			sa.score = d_r[0]; sa.end_i = d_r[1]; sa.end_j = d_r[2]; sa.state = d_r[3];
			sa.key = d_pkey; sa.bad = lb.bad;
			sa.o_score = d_r[4]; sa.o_end_i = d_r[5]; sa.o_end_j = d_r[6]; sa.o_state = d_r[7];
			HIP_TRY(h, at_tilescan_init_launch(&sa, h->ncu, s));
			for (int pass = 0; pass < 2; ++pass) {
				const long long tall = tpre[pass][(size_t)B.ntb];
				if (tall == 0) continue;
				auto items_before = [&](int64_t x) { return (long long)(x / B.ntb) * tall + tpre[pass][(size_t)(x % B.ntb)]; };
				const long long ya = items_before(p0), yb = items_before(p0 + n);
				sa.ragged = pass; sa.tall = tall; sa.tpre = d_tpre[pass];
				for (long long y = ya; y < yb; y += chunk) {
					sa.y0 = y; sa.nitems = std::min<long long>(chunk, yb - y);
					HIP_TRY(h, at_tilescan_desc_launch(F.mode, &sa, h->ncu, s));
					BatchReq r(h);
					r.mode = F.mode; r.npairs = sa.nitems; r.d_seq = rs.d_words; r.bits = rs.bits; r.stream = s;
					r.d_woff1 = d_woff1; r.d_len1 = d_len1; r.d_woff2 = d_woff2; r.d_len2 = d_len2;
					r.max_len1 = B.l1; r.max_len2 = pass ? bt.rag_most : (int32_t)(tile + ov);
					r.uniform_shape = pass ? 0 : 1;
					r.d_score = d_r[0]; r.d_end_i = d_r[1]; r.d_end_j = d_r[2]; r.d_state = d_r[3];
					rc = align_device(h, r);
					if (rc) { (void)hipStreamSynchronize(s); return rc; }
					if (nslices == 0) cfg0 = h->cfg;
					HIP_TRY(h, at_tilescan_fold_launch(F.mode, &sa, h->ncu, s));
					++nslices;
				}
			}
			HIP_TRY(h, at_tilescan_unpack_launch(F.mode, &sa, h->ncu, s));
			if ((rc = merge_slice(h, qo, lb, d_qperm, d_tperm, d_r + 4, p0, n, B.ntb, B.qa, B.ta, k, 0, use_cutoff, cutoff))) return rc;
		}
	}
	HIP_TRY(h, hipEventRecord(ev.e[1], s));
	if ((rc = lists_readback(h, lb, nq, k, qo.enc, false, F.who, out))) return rc;
	float sweep_ms = 0.f;
	HIP_TRY(h, hipEventElapsedTime(&sweep_ms, ev.e[0], ev.e[1]));
	/* (the sweep phase's device time as scan_lists reports it: tools/local_scan_rate.py, tools/fit_scan_rate.py; at most 360 bytes, which
	 * tilescan_cigars keeps whole) */
	if (F.mode == AT_MODE_FIT)
		snprintf(h->cfg, sizeof h->cfg, "scan-fit: tile=%d overlap=%lld tiles=%lld strands=%s, %lld blocks, %lld slices, k=%d; %.200s sweep=%.3fms", tile,
		         (long long)ov_most, (long long)tiles_all, scan_strands_text(strands), (long long)blocks.size(), (long long)nslices, k, cfg0.c_str(), (double)sweep_ms);
	else
		snprintf(h->cfg, sizeof h->cfg, "local-scan: tile=%d overlap<=%lld tiles=%lld k=%d strands=%s, %lld blocks, %lld slices; %.200s sweep=%.3fms", tile,
		         (long long)ov_most, (long long)tiles_all, k, scan_strands_text(strands), (long long)blocks.size(), (long long)nslices, cfg0.c_str(), (double)sweep_ms);
	return AT_OK;
}

/* the alignments of the hits: every USED list entry as a window pair (query, target columns of the hit's window) through the batch
 * entry with tracebacks and the CIGAR kernels (at_tilescan.hip.h), in pieces of at most 2^20 hits or 1 GB of op slots (3.13's bounds)
 * and no more hits than a slice has pairs (AT_ALLPAIRS_CHUNK: the tests' 1 and 7 make pieces of 1 and 7 hits).  Unused entries keep
 * what the entry gave them: 0 runs, a row of -1 and no room in out_cigar */
static int tilescan_cigars(at_handle *h, const TileScanFamily &F, const QuerySets &qt, int k, int strands, const ReadSet &rs, int32_t maxq, const ListBufs &lb,
                           const ListOut &out, int flags, const CigarOut &co)
{
	const int64_t nq = qt.nq, nt = qt.nt, nlist = nq * k;
	std::vector<long long> used;
	std::vector<int32_t> wlen;
	for (int64_t e = 0; e < nlist; ++e) {
		if (out.target[e] < 0) continue;
		used.push_back(e);
		wlen.push_back(F.window_len(h, qt.q_len[e / k], qt.t_len[out.target[e]], out.score[e], out.end_i[e], out.end_j[e]));
	}
	const int64_t nused = (int64_t)used.size();
	const int64_t piece_hits = std::max<long long>(1, std::min<long long>(env_ll("AT_ALLPAIRS_CHUNK", at::kSliceDefault), 1LL << 20)), piece_ops = 1LL << 30;
	hipStream_t s = h->stream;
	const std::string cfg0 = h->cfg;
	std::string cfg1;
	int64_t words_total = 0, npieces = 0;   /* CIGAR words of the hits so far: the next piece's place in out_cigar */
	bool fits = true;                        /* every entry so far ends within the caller's capacity */
	int64_t next_entry = 0;                  /* out_cigar_off is complete up to here */
	for (int64_t a0 = 0; a0 < nused; ) {
		int64_t ops_bytes = 0;
		const int64_t n = at::piece_end(a0, nused, piece_hits, piece_ops, [&](int64_t x) { return (int64_t)maxq + wlen[(size_t)x]; }, &ops_bytes) - a0;
		int32_t max2 = 1;
		std::vector<int64_t> slot((size_t)n);
		for (int64_t x = 0, at = 0; x < n; at += (int64_t)maxq + wlen[(size_t)(a0 + x)], ++x) {
			slot[(size_t)x] = at;
			max2 = std::max(max2, wlen[(size_t)(a0 + x)]);
		}
		const int64_t dcap = std::min<int64_t>(std::max<int64_t>(co.cap - words_total, 0), ops_bytes);   /* (a list has no more runs than ops) */
		char bad_text[256];
		if (F.mode == AT_MODE_FIT)
			snprintf(bad_text, sizeof bad_text, "at_scan_fit: a hit's window does not reproduce its score, state and end column (target columns (ws, we] of at most %d)", max2);
		else
			snprintf(bad_text, sizeof bad_text, "at_scan_local: a hit's window does not reproduce its score and end cell (target columns (ws, j*] of at most %d)", max2);
		std::vector<int32_t> hnc((size_t)n), hst((size_t)n * 8);
		std::vector<int64_t> hco((size_t)n + 1);
		WindowBufs w;
		int rc = window_carve(h, n, dcap, 0, true, false, &h->d_order, &h->order_bytes, (size_t)ops_bytes + 256, w);
		if (rc) return rc;
		HIP_TRY(h, hipMemcpyAsync(w.ops_off, slot.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
		HIP_TRY(h, hipMemcpyAsync(w.eidx, used.data() + a0, (size_t)n * 8, hipMemcpyHostToDevice, s));
		HIP_TRY(h, hipMemsetAsync(w.bad, 0, 4, s));
		at::TileScanWindowArgs wa;
		memset(&wa, 0, sizeof wa);
		wa.n = n; wa.nlist = nlist; wa.eidx = w.eidx; wa.k = k; wa.nq = (int)nq; wa.enc = strands != AT_STRAND_FWD; wa.nrev0 = (int)(nq + nt);
		wa.bpw = rs.bits == 2 ? 16 : 4;
		wa.m = h->m; wa.u = h->u; wa.o = h->o; wa.e = h->e;
		wa.lkey = lb.key; wa.lei = lb.ei; wa.lej = lb.ej; wa.lst = lb.st;
		wa.swoff = (const long long *)rs.d_swoff; wa.slen = rs.d_len;
		wa.woff1 = (long long *)w.woff1; wa.woff2 = (long long *)w.woff2; wa.len1 = w.len1; wa.len2 = w.len2; wa.ws = w.aux;
		wa.w_score = w.sc; wa.w_end_i = w.ei; wa.w_end_j = w.ej; wa.w_state = w.st; wa.ncigar = w.ncigar; wa.stats = w.stats; wa.bad = w.bad;
		HIP_TRY(h, at_tilescan_window_launch(F.mode, &wa, h->ncu, s));
		rc = align_device(h, window_req(h, F.mode, n, rs, w, maxq, max2, s));
		if (rc) { (void)hipStreamSynchronize(s); return rc; }
		if (cfg1.empty()) cfg1 = h->cfg;
		rc = at_cigar_batch_device(h, n, rs.d_words, rs.bits, w.woff1, w.woff2, w.ei, w.ej, w.ops, w.ops_off, w.nops, flags, w.ncigar, w.stats, w.coff, w.cigar, dcap, s);
		if (rc) { (void)hipStreamSynchronize(s); return rc; }
		HIP_TRY(h, at_tilescan_check_launch(F.mode, &wa, h->ncu, s));
		if ((rc = window_fetch(h, w, n, bad_text, hnc.data(), hst.data(), hco.data()))) return rc;
		for (int64_t x = 0; x < n; ++x) {
			const int64_t e = used[(size_t)(a0 + x)];
			for (; next_entry <= e; ++next_entry) co.off[next_entry] = words_total + hco[(size_t)x];
			co.ncigar[e] = hnc[(size_t)x];
			memcpy(co.stats + e * 8, hst.data() + x * 8, 32);
		}
		/* the piece's words that end within the caller's capacity: a prefix of the device buffer, behind the pieces before it */
		const int64_t room = fits ? co.cap - words_total : 0;
		if ((rc = window_words(h, w, hco.data(), n, room, room > 0 ? co.words + words_total : nullptr))) return rc;
		fits = fits && hco[(size_t)n] <= room;
		words_total += hco[(size_t)n];
		a0 += n;
		++npieces;
	}
	for (; next_entry <= nlist; ++next_entry) co.off[next_entry] = words_total;
	snprintf(h->cfg, sizeof h->cfg, "%.360s; windows: %.180s, %lld pieces, cigars: %d lanes/pair", cfg0.c_str(), cfg1.c_str(), (long long)npieces, h->last_cigar_lanes);
	return AT_OK;
}

/* the body of at_scan_local and at_scan_fit: the shared refusals with the family's own in between, in the order each entry always had */
static int tilescan_entry(at_handle *h, const TileScanFamily &F, const QuerySets &qt, int k, int use_cutoff, int32_t cutoff, int strands, int32_t tile_cols,
                          int flags, const ListOut &out, const CigarOut &co)
{
	const char *who = F.who;
	if (!h) return fail(nullptr, AT_ERR_ARG, "%s: NULL handle", who);
	const int64_t nq = qt.nq, nt = qt.nt;
	int rc = check_sizes(h, who, nq, nt, co.cap, k);
	if (rc || (rc = check_options(h, who, strands, tile_cols, F.default_tile, flags, co, nq, nt)) || (rc = check_one_gpu(h, who))) return rc;
	const bool rev = strands != AT_STRAND_FWD;
	if ((rc = F.check_scoring(h))) return rc;
	if (nq == 0) return AT_OK;
	if ((rc = check_list_pointers(h, who, qt, out, rev))) return rc;
	int32_t maxq = 0;
	for (int64_t q = 0; q < nq; ++q) {
		if ((rc = check_read(h, "query", q, qt.q_len[q], qt.q_off[q], true)) || (rc = F.check_query(h, q, qt.q_len[q]))) return rc;
		maxq = std::max(maxq, qt.q_len[q]);
	}
	for (int64_t t = 0; t < nt; ++t) if ((rc = check_read(h, "target", t, qt.t_len[t], qt.t_off[t], F.target_need_base))) return rc;
	const int32_t tile = tile_cols > 0 ? tile_cols : F.default_tile;
	return guarded(h, who, [&]() -> int {
		list_out_init(out, nq, k, co);
		if (nt == 0) {
			if (F.mode == AT_MODE_FIT)
				snprintf(h->cfg, sizeof h->cfg, "scan-fit: tile=%d overlap=0 tiles=0 strands=%s, 0 blocks, 0 slices, k=%d; ", tile, scan_strands_text(strands), k);
			else
				snprintf(h->cfg, sizeof h->cfg, "local-scan: tile=%d overlap<=0 tiles=0 k=%d strands=%s, 0 blocks, 0 slices; ", tile, k, scan_strands_text(strands));
			return (int)AT_OK;
		}
		ReadSet rs;
		int rc2 = upload_sets(h, F.mode, qt, rev, &rs);
		if (rc2) return rc2;
		ListBufs lb;
		if ((rc2 = tilescan_lists(h, F, qt, rs, k, use_cutoff, cutoff, strands, tile, out, lb)) || !co.any()) return rc2;
		return tilescan_cigars(h, F, qt, k, strands, rs, maxq, lb, out, flags, co);
	});
}

extern "C" int at_scan_local(at_handle *h,
                             int64_t nq, const uint8_t *q_blob, const int64_t *q_off, const int32_t *q_len,
                             int64_t nt, const uint8_t *t_blob, const int64_t *t_off, const int32_t *t_len,
                             int k, int use_cutoff, int32_t cutoff, int strands, int32_t tile_cols, int flags,
                             int32_t *out_target, int32_t *out_score, int32_t *out_end_i, int32_t *out_end_j,
                             int32_t *out_state, int32_t *out_strand, int32_t *out_nhits,
                             int32_t *out_stats, int32_t *out_ncigar, int64_t *out_cigar_off,
                             uint32_t *out_cigar, int64_t cigar_cap)
{
	return tilescan_entry(h, kScanLocal, {nq, q_blob, q_off, q_len, nt, t_blob, t_off, t_len}, k, use_cutoff, cutoff, strands, tile_cols, flags,
	                      {out_target, out_score, out_end_i, out_end_j, out_state, out_strand, out_nhits},
	                      {out_stats, out_ncigar, out_cigar_off, out_cigar, cigar_cap});
}

extern "C" int at_scan_fit(at_handle *h,
                           int64_t nq, const uint8_t *q_blob, const int64_t *q_off, const int32_t *q_len,
                           int64_t nt, const uint8_t *t_blob, const int64_t *t_off, const int32_t *t_len,
                           int k, int use_cutoff, int32_t cutoff, int strands, int32_t tile_cols, int flags,
                           int32_t *out_target, int32_t *out_score, int32_t *out_end_i, int32_t *out_end_j,
                           int32_t *out_state, int32_t *out_strand, int32_t *out_nhits,
                           int32_t *out_stats, int32_t *out_ncigar, int64_t *out_cigar_off,
                           uint32_t *out_cigar, int64_t cigar_cap)
{
	return tilescan_entry(h, kScanFit, {nq, q_blob, q_off, q_len, nt, t_blob, t_off, t_len}, k, use_cutoff, cutoff, strands, tile_cols, flags,
	                      {out_target, out_score, out_end_i, out_end_j, out_state, out_strand, out_nhits},
	                      {out_stats, out_ncigar, out_cigar_off, out_cigar, cigar_cap});
}

/* ---- every occurrence of a read under a distance cutoff (at_scan_hits; at_scanhits.hip.h) ---- */
struct ScanHitsRun {
	long long cand = 0, kept = 0, resweeps = 0, nslices = 0, nblocks = 0, gall = 0;
	int ov_most = 0;
	double sweep_ms = 0.0, select_ms = 0.0;
	std::string cfg0;
};

/* the hits of at_scan_hits in their final order and the hits of each query: the blocks and slices of scan_lists; per slice the groups
 * of its pairs are swept by at_scan<W, true> (once more into a buffer of the counted size if the candidates did not fit), the
 * candidates sorted, marked and compacted on the device (at_scanhits.hip.h) and the kept ones fetched */
static int scan_hits_lists(at_handle *h, const QuerySets &qt, const ReadSet &rs, int32_t max_dist, int32_t min_sep, int strands, int32_t tile,
                           int64_t cand_cap, std::vector<at::ScanHit> &hits, std::vector<int32_t> &qcount, ScanHitsRun &run)
{
	const int64_t nq = qt.nq, nt = qt.nt;
	const at::QueryOrder qo = at::query_order(nq, qt.q_len, strands);
	ScanSweep sw(qt, qo.enc, tile, rs);
	int64_t tsum = 0, most = 0;
	for (int64_t t = 0; t < nt; ++t) tsum += qt.t_len[t];
	std::vector<at::QueryBlock> blocks;
	for (const at::QueryBlock &B : qo.blocks) {
		if (B.l1 < 1) continue;                                   /* a query of length 0 has no hits */
		blocks.push_back(B);
		most = std::max<int64_t>(most, (int64_t)B.nqb * nt);
	}
	const int64_t chunk = at::slice_clamp(env_ll("AT_ALLPAIRS_CHUNK", at::kSliceDefault), most);
	unsigned long long *d_ncand = nullptr; long long *d_gpre = nullptr; int *d_qperm = nullptr, *d_qcount = nullptr;
	int rc = carve(h, &h->d_desc, &h->desc_bytes, [&](Carver &c) {
		d_ncand = c.take<unsigned long long>(1); d_gpre = c.take<long long>((size_t)nt + 1);
		d_qperm = c.take<int>((size_t)qo.nv); d_qcount = c.take<int>((size_t)nq);
	});
	if (rc) return rc;
	hipStream_t s = h->stream;
	HIP_TRY(h, hipMemcpyAsync(d_qperm, qo.qperm.data(), (size_t)qo.nv * 4, hipMemcpyHostToDevice, s));
	HIP_TRY(h, hipMemcpyAsync(d_gpre, sw.gpre.data(), ((size_t)nt + 1) * 8, hipMemcpyHostToDevice, s));
	HIP_TRY(h, hipMemsetAsync(d_qcount, 0, (size_t)nq * 4, s));
	/* the candidate block of a capacity: keys and values before and behind the sort, prefix sums, flags, hit records */
	struct Cand { unsigned long long *k0, *k1; long long *off; int *v0, *v1, *flag; at::ScanHit *hit; } cd = {};
	auto cand_carve = [&](int64_t cap) {
		return carve(h, &h->d_cand, &h->cand_bytes, [&](Carver &c) {
			cd.k0 = c.take<unsigned long long>((size_t)cap); cd.k1 = c.take<unsigned long long>((size_t)cap); cd.off = c.take<long long>((size_t)cap + 1);
			cd.v0 = c.take<int>((size_t)cap); cd.v1 = c.take<int>((size_t)cap); cd.flag = c.take<int>((size_t)cap); cd.hit = c.take<at::ScanHit>((size_t)cap);
		});
	};
	StreamEvents ev;
	if ((rc = ev.create(h, 3))) return rc;
	run.gall = sw.gall; run.nblocks = (long long)blocks.size();
	for (const at::QueryBlock &B : blocks) {
		const int64_t bp = (int64_t)B.nqb * nt;
		if ((rc = sw.block(h, B.l1, at_scan_hits_kernel))) return rc;
		const int32_t c = at::scan_hits_bound(B.l1, max_dist);
		run.ov_most = std::max(run.ov_most, (int)at::scan_overlap(B.l1, 1, c));
		for (int64_t s0 = 0; s0 < bp; s0 += chunk) {
			const int64_t n = std::min(chunk, bp - s0);
			/* no pair has more candidates than its target has columns */
			const long double mc = ((long double)(n / nt) + 2.0L) * (long double)tsum;   /* (the slice touches at most n / nt + 2 entries) */
			const int64_t most_cand = mc > 4e18L ? (int64_t)4e18L : std::max<int64_t>(1, (int64_t)mc);
			int64_t cap = std::min<int64_t>(cand_cap > 0 ? cand_cap : at::kScanHitsDefaultCand, most_cand);
			at::ScanArgs sa = sw.slice(B.qa, s0, n, d_gpre, d_qperm, 1, c);
			const long long grid = sw.grid(h, sa);
			unsigned long long ncand = 0;
			for (int turn = 0;; ++turn) {
				if ((rc = cand_carve(cap))) return rc;
				sa.cand_n = d_ncand; sa.cand_cap = cap; sa.cand_key = cd.k0; sa.cand_val = cd.v0;
				HIP_TRY(h, hipMemsetAsync(d_ncand, 0, 8, s));
				if (int rcq = ensure_queue(h, s)) return rcq;
				sa.queue = h->d_queue;
				HIP_TRY(h, hipEventRecord(ev.e[0], s));
				HIP_TRY(h, at_scan_hits_launch(&sa, sw.w, (unsigned)grid, s));
				HIP_TRY(h, hipEventRecord(ev.e[1], s));
				HIP_TRY(h, hipMemcpyAsync(&ncand, d_ncand, 8, hipMemcpyDeviceToHost, s));
				HIP_TRY(h, hipStreamSynchronize(s));
				float ms = 0.f;
				HIP_TRY(h, hipEventElapsedTime(&ms, ev.e[0], ev.e[1]));
				run.sweep_ms += ms;
				if (ncand <= (unsigned long long)cap) break;
				/* they did not fit: the buffer goes, one of the counted size comes and the slice is swept once more (the count of a
				 * slice does not depend on the order of its appends, so the second sweep fits) */
				if (turn > 0 || ncand > (unsigned long long)most_cand)
					return fail(h, AT_ERR_RANGE, "at_scan_hits: a slice counted %llu candidates after %lld", ncand, (long long)cap);
				if (h->d_cand) { (void)hipFree(h->d_cand); h->d_cand = nullptr; h->cand_bytes = 0; }
				cap = (int64_t)ncand;
				++run.resweeps;
			}
			if (run.nslices == 0) run.cfg0 = sw.text("myers-scan-hits", grid);
			++run.nslices;
			run.cand += (long long)ncand;
			if (ncand == 0) continue;
			const long long nc = (long long)ncand;
			size_t tmp_bytes = 0;
			HIP_TRY(h, at_scanhits_sort(nullptr, &tmp_bytes, cd.k0, cd.k1, cd.v0, cd.v1, nc, n, s));
			rc = grow(h, &h->d_sorttmp, &h->sorttmp_bytes, std::max<size_t>(tmp_bytes, 256));
			if (rc) return rc;
			HIP_TRY(h, at_scanhits_sort(h->d_sorttmp, &tmp_bytes, cd.k0, cd.k1, cd.v0, cd.v1, nc, n, s));
			at::ScanHitsArgs ha;
			memset(&ha, 0, sizeof ha);
			ha.n = nc; ha.key = cd.k1; ha.val = cd.v1; ha.s0 = s0; ha.ntb = nt; ha.qa = B.qa; ha.enc = qo.enc; ha.nrev0 = (int)(nq + nt);
			ha.min_sep = min_sep; ha.qperm = d_qperm; ha.slen = rs.d_len; ha.flag = cd.flag; ha.off = cd.off; ha.hits = cd.hit; ha.qcount = d_qcount;
			HIP_TRY(h, at_scanhits_mark_launch(&ha, h->ncu, s));
			rc = scan_nops_device(h, nc, cd.flag, (int64_t *)cd.off, s);
			if (rc) return rc;
			HIP_TRY(h, at_scanhits_emit_launch(&ha, h->ncu, s));
			HIP_TRY(h, hipEventRecord(ev.e[2], s));
			long long kept = 0;
			HIP_TRY(h, hipMemcpyAsync(&kept, cd.off + nc, 8, hipMemcpyDeviceToHost, s));
			HIP_TRY(h, hipStreamSynchronize(s));
			float ms = 0.f;
			HIP_TRY(h, hipEventElapsedTime(&ms, ev.e[1], ev.e[2]));
			run.select_ms += ms;
			if (kept < 0 || kept > nc) return fail(h, AT_ERR_RANGE, "at_scan_hits: %lld hits kept of %lld candidates", kept, nc);
			if (kept > 0) {
				const size_t was = hits.size();
				hits.resize(was + (size_t)kept);
				HIP_TRY(h, hipMemcpyAsync(hits.data() + was, cd.hit, (size_t)kept * sizeof(at::ScanHit), hipMemcpyDeviceToHost, s));
				HIP_TRY(h, hipStreamSynchronize(s));
			}
			run.kept += kept;
		}
	}
	qcount.assign((size_t)nq, 0);
	if (nq > 0) {
		HIP_TRY(h, hipMemcpyAsync(qcount.data(), d_qcount, (size_t)nq * 4, hipMemcpyDeviceToHost, s));
		HIP_TRY(h, hipStreamSynchronize(s));
	}
	at::scan_hits_order(hits.data(), (int64_t)hits.size());
	return AT_OK;
}

extern "C" int at_scan_hits(at_handle *h,
                            int64_t nq, const uint8_t *q_blob, const int64_t *q_off, const int32_t *q_len,
                            int64_t nt, const uint8_t *t_blob, const int64_t *t_off, const int32_t *t_len,
                            int32_t max_dist, int32_t min_sep, int strands, int32_t tile_cols, int64_t cand_cap, int flags,
                            int64_t hit_cap, int64_t *out_hit_off,
                            int32_t *out_target, int32_t *out_score, int32_t *out_end_j, int32_t *out_strand,
                            int32_t *out_stats, int32_t *out_ncigar, int64_t *out_cigar_off, uint32_t *out_cigar, int64_t cigar_cap)
{
	const char *who = "at_scan_hits";
	if (!h) return fail(nullptr, AT_ERR_ARG, "at_scan_hits: NULL handle");
	const QuerySets qt = {nq, q_blob, q_off, q_len, nt, t_blob, t_off, t_len};
	const CigarOut co = {out_stats, out_ncigar, out_cigar_off, out_cigar, cigar_cap};
	int rc = check_sizes(h, who, nq, nt, cigar_cap);
	if (rc) return rc;
	if (max_dist < 0) return fail(h, AT_ERR_ARG, "at_scan_hits: max_dist = %d is negative", max_dist);
	if (min_sep < AT_SCAN_SEP_READ) return fail(h, AT_ERR_ARG, "at_scan_hits: min_sep = %d (a distance in columns, 0, or AT_SCAN_SEP_READ)", min_sep);
	if (cand_cap < 0 || hit_cap < 0) return fail(h, AT_ERR_ARG, "at_scan_hits: negative capacity");
	if ((rc = check_options(h, who, strands, tile_cols, at::kScanDefaultTile, flags, co, nq, nt)) || (rc = check_one_gpu(h, who))) return rc;
	const bool rev = strands != AT_STRAND_FWD, cg = co.any();
	if (h->u != 1) return fail(h, AT_ERR_DOMAIN, "at_scan_hits needs the unit mismatch cost: u = %d, not 1", h->u);
	if (!out_hit_off || (nq > 0 && (!q_blob || !q_off || !q_len || (nt > 0 && (!t_blob || !t_off || !t_len)))) ||
	    (hit_cap > 0 && (!out_target || !out_score || !out_end_j || (rev && !out_strand))))
		return fail(h, AT_ERR_ARG, "at_scan_hits: NULL argument");
	int32_t maxq = 0;
	for (int64_t q = 0; q < nq; ++q) {
		if ((rc = check_read(h, "query", q, q_len[q], q_off[q], false))) return rc;
		if (q_len[q] > at::kScanMaxQuery) return fail(h, AT_ERR_DOMAIN, "at_scan_hits: query %lld has %d bases, more than %d", (long long)q, q_len[q], at::kScanMaxQuery);
		maxq = std::max(maxq, q_len[q]);
	}
	for (int64_t t = 0; t < nt; ++t) if ((rc = check_read(h, "target", t, t_len[t], t_off[t], false))) return rc;
	const int32_t tile = tile_cols > 0 ? tile_cols : at::kScanDefaultTile;
	return guarded(h, who, [&]() -> int {
		for (int64_t q = 0; q <= nq; ++q) out_hit_off[q] = 0;
		ScanHitsRun run;
		auto config = [&]() {
			snprintf(h->cfg, sizeof h->cfg, "scan-hits: tile=%d overlap<=%d groups=%lld max_dist=%d min_sep=%d strands=%s, %lld blocks, %lld slices, "
			         "candidates=%lld kept=%lld resweeps=%lld; %s sweep=%.3fms select=%.3fms", tile, run.ov_most, run.gall, max_dist, min_sep,
			         scan_strands_text(strands), run.nblocks, run.nslices, run.cand, run.kept, run.resweeps, run.cfg0.c_str(), run.sweep_ms, run.select_ms);
		};
		if (nq == 0 || nt == 0) {
			if (cg && hit_cap >= 0) out_cigar_off[0] = 0;
			config();
			return (int)AT_OK;
		}
		ReadSet rs;
		int rc = upload_sets(h, AT_MODE_EDIT, qt, rev, &rs);
		if (rc) return rc;
		if (rs.bits != 2) return fail(h, AT_ERR_DOMAIN, "at_scan_hits needs 2-bit reads: some base of a query or a target is not one of ACGT");
		std::vector<at::ScanHit> hits;
		std::vector<int32_t> qcount;
		rc = scan_hits_lists(h, qt, rs, max_dist, min_sep, strands, tile, cand_cap, hits, qcount, run);
		if (rc) return rc;
		config();
		const int64_t nh = (int64_t)hits.size();
		for (int64_t q = 0; q < nq; ++q) out_hit_off[q + 1] = out_hit_off[q] + qcount[(size_t)q];
		if (out_hit_off[nq] != nh) return fail(h, AT_ERR_RANGE, "at_scan_hits: %lld hits fetched, %lld counted", (long long)nh, (long long)out_hit_off[nq]);
		if (nh > hit_cap) return (int)AT_OK;               /* the caller comes back with room */
		for (int64_t e = 0; e < nh; ++e) {
			const at::ScanHit &x = hits[(size_t)e];
			out_target[e] = x.target; out_score[e] = x.score; out_end_j[e] = x.end_j;
			if (out_strand) out_strand[e] = x.strand;
		}
		if (!cg) return (int)AT_OK;
		out_cigar_off[0] = 0;
		if (nh == 0) return (int)AT_OK;
		/* the window pass over the hits, in pieces that keep its descriptor and op buffers moderate: each piece as lists of its own
		 * (key, query, end column of every hit) */
		std::vector<unsigned long long> lkey;
		std::vector<int32_t> lej, leq, lei;
		std::vector<int64_t> p_off;
		std::string wcfg;
		for (int64_t a = 0, b; a < nh; a = b) {
			b = at::piece_end(a, nh, 1LL << 20, 1LL << 30, [&](int64_t e) { return 2LL * q_len[hits[(size_t)e].query] + hits[(size_t)e].score + 16; });
			const int64_t n = b - a;
			lkey.assign((size_t)n, 0); lej.assign((size_t)n, 0); leq.assign((size_t)n, 0); lei.assign((size_t)n, 0);
			for (int64_t e = 0; e < n; ++e) {
				const at::ScanHit &x = hits[(size_t)(a + e)];
				lkey[(size_t)e] = at::list_key(-x.score, x.target, x.strand, rev);
				lej[(size_t)e] = x.end_j; leq[(size_t)e] = x.query; lei[(size_t)e] = q_len[x.query];
			}
			ListBufs lb;
			if ((rc = list_bufs(h, (size_t)n, false, &lb))) return rc;
			hipStream_t s = h->stream;
			HIP_TRY(h, hipMemcpyAsync(lb.key, lkey.data(), (size_t)n * 8, hipMemcpyHostToDevice, s));
			HIP_TRY(h, hipMemcpyAsync(lb.ei, leq.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
			HIP_TRY(h, hipMemcpyAsync(lb.ej, lej.data(), (size_t)n * 4, hipMemcpyHostToDevice, s));
			HIP_TRY(h, hipStreamSynchronize(s));
			const int64_t base = out_cigar_off[a];
			p_off.assign((size_t)n + 1, 0);
			const int64_t room = std::max<int64_t>(0, cigar_cap - base);
			const CigarOut piece = {out_stats + a * 8, out_ncigar + a, p_off.data(), room > 0 ? out_cigar + base : nullptr, room};
			rc = scan_cigars(h, nq, 1, strands, rs, nt, maxq, lb, out_target + a, out_score + a, lei.data(), out_end_j + a, flags, piece, n, who);
			if (rc) return rc;
			for (int64_t e = 1; e <= n; ++e) out_cigar_off[a + e] = base + p_off[(size_t)e];
			if (wcfg.empty()) { const char *w = strstr(h->cfg, "; windows: "); wcfg = w ? w : ""; }
		}
		config();
		cfg_append(h, "%s", wcfg.c_str());
		return (int)AT_OK;
	});
}

/* ---- reverse complement: the host helper and the device entry (the kernel: at_revcomp.hip) ---- */
extern "C" int at_revcomp(const uint8_t *s, int32_t len, uint8_t *out)
{
	static constexpr at::CompTable comp = at::make_comp_table();
	if (len < 0 || (len > 0 && (!s || !out))) return fail(nullptr, AT_ERR_ARG, "at_revcomp: NULL argument or negative length");
	for (int32_t x = 0; x < len; ++x) out[x] = comp.t[s[len - 1 - x]];
	return AT_OK;
}

extern "C" int at_revcomp_device(at_handle *h, int64_t nseq, const uint32_t *d_seq, int bits,
                                 const int64_t *d_woff, const int32_t *d_len,
                                 uint32_t *d_out, const int64_t *d_out_woff, void *stream)
{
	if (!h) return fail(nullptr, AT_ERR_ARG, "at_revcomp_device: NULL handle");
	if (nseq < 0) return fail(h, AT_ERR_ARG, "negative nseq");
	if (bits != 2 && bits != 8) return fail(h, AT_ERR_ARG, "bits must be 2 or 8");
	if (nseq == 0) return AT_OK;
	if (!d_seq || !d_woff || !d_len || !d_out) return fail(h, AT_ERR_ARG, "NULL device pointer");
	HIP_TRY(h, hipSetDevice(h->device));
	drop_stale_error();
	at::RevcompArgs ra;
	ra.nseq = nseq; ra.seq = d_seq; ra.woff = (const long long *)d_woff; ra.len = d_len;
	ra.out = d_out; ra.out_woff = (const long long *)(d_out_woff ? d_out_woff : d_woff);
	HIP_TRY(h, at_revcomp_launch(&ra, bits, h->ncu, (hipStream_t)stream));
	return AT_OK;
}

namespace {
struct CopyOut { int64_t first; int32_t *score, *end_i, *end_j, *state; };
int copy_out_slice(void *user, int64_t first, int64_t n, const int32_t *sc, const int32_t *ei, const int32_t *ej, const int32_t *st)
{
	const CopyOut *o = (const CopyOut *)user;
	const size_t at = (size_t)(first - o->first), nb = (size_t)n * 4;
	memcpy(o->score + at, sc, nb);
	if (o->end_i) memcpy(o->end_i + at, ei, nb);
	if (o->end_j) memcpy(o->end_j + at, ej, nb);
	if (o->state) memcpy(o->state + at, st, nb);
	return 0;
}
}

/* one slice of the triangle WITH tracebacks: ops of pair p go to the caller's slot ops_off[p - first_pair] */
static int allpairs_tb_slice(at_handle *h, int mode, int64_t nreads, const ReadSet &rs, int64_t first_pair, int64_t npairs,
                             int32_t *out_score, int32_t *out_end_i, int32_t *out_end_j, int32_t *out_state,
                             uint8_t *out_ops, const int64_t *ops_off, int32_t *out_nops)
{
	const int maxlen = rs.maxlen;
	int64_t ops_total = 0, ops_lo = INT64_MAX;
	for (int64_t p = 0; p < npairs; ++p) { if (ops_off[p] < 0) return fail(h, AT_ERR_ARG, "pair %lld: negative ops offset", (long long)(first_pair + p)); ops_lo = std::min(ops_lo, ops_off[p]); }
	std::vector<int64_t> opsr((size_t)npairs);
	for (int64_t p = 0; p < npairs; ++p) { opsr[(size_t)p] = ops_off[p] - ops_lo; ops_total = std::max<int64_t>(ops_total, opsr[(size_t)p] + 2LL * maxlen); }
	const int64_t slots_total = npairs * 2LL * maxlen;
	auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
	int rc = grow(h, &h->d_desc, &h->desc_bytes, al((size_t)npairs * 8));
	if (rc) return rc;
	int64_t *d_opsoff = (int64_t *)h->d_desc;
	hipStream_t s = h->stream;
	HIP_TRY(h, hipMemcpyAsync(d_opsoff, opsr.data(), (size_t)npairs * 8, hipMemcpyHostToDevice, s));
	const size_t b_res = al((size_t)npairs * 4), b_ops = al((size_t)ops_total + 64), b_pfx = al((size_t)(npairs + 1) * 8);
	rc = grow(h, &h->d_out, &h->out_bytes, 5 * b_res + b_ops + b_pfx);
	if (rc) return rc;
	char *dout = (char *)h->d_out;
	int32_t *d_score = (int32_t *)dout, *d_ei = (int32_t *)(dout + b_res), *d_ej = (int32_t *)(dout + 2 * b_res);
	int32_t *d_st = (int32_t *)(dout + 3 * b_res), *d_nops = (int32_t *)(dout + 4 * b_res);
	uint8_t *d_ops = (uint8_t *)(dout + 5 * b_res);
	int64_t *d_poff = (int64_t *)(dout + 5 * b_res + b_ops);
	BatchReq r = triangle_req(h, mode, rs, nreads, first_pair, npairs, s);
	r.want_traceback = 1;
	r.d_score = d_score; r.d_end_i = d_ei; r.d_end_j = d_ej; r.d_state = d_st;
	r.d_ops = d_ops; r.d_ops_off = d_opsoff; r.d_nops = d_nops;
	rc = align_device(h, r);
	if (rc) return rc;
	HIP_TRY(h, hipMemcpyAsync(out_score, d_score, (size_t)npairs * 4, hipMemcpyDeviceToHost, s));
	if (out_end_i) HIP_TRY(h, hipMemcpyAsync(out_end_i, d_ei, (size_t)npairs * 4, hipMemcpyDeviceToHost, s));
	if (out_end_j) HIP_TRY(h, hipMemcpyAsync(out_end_j, d_ej, (size_t)npairs * 4, hipMemcpyDeviceToHost, s));
	if (out_state) HIP_TRY(h, hipMemcpyAsync(out_state, d_st, (size_t)npairs * 4, hipMemcpyDeviceToHost, s));
	HIP_TRY(h, hipMemcpyAsync(out_nops, d_nops, (size_t)npairs * 4, hipMemcpyDeviceToHost, s));
	rc = grow(h, &h->d_str, &h->str_bytes, al((size_t)slots_total + 64));
	if (rc) return rc;
	rc = at_compact_ops_device(h, npairs, d_ops, d_opsoff, d_nops, (uint8_t *)h->d_str, slots_total, d_poff, s);
	if (rc) return rc;
	std::vector<int64_t> h_poff((size_t)npairs + 1);
	HIP_TRY(h, hipMemcpyAsync(h_poff.data(), d_poff, (size_t)(npairs + 1) * 8, hipMemcpyDeviceToHost, s));
	HIP_TRY(h, hipStreamSynchronize(s));
	for (int64_t p = 0; p < npairs; ++p)
		if (out_score[p] == INT32_MIN || out_nops[p] < 0)
			return fail(h, AT_ERR_DOMAIN, "pair %lld: input outside the domain on which the reference is defined", (long long)(first_pair + p));
	const int64_t total = h_poff[(size_t)npairs];
	if (total < 0 || total > slots_total) return fail(h, AT_ERR_DOMAIN, "traceback lengths inconsistent with the slots");
	std::vector<uint8_t> pk((size_t)total + 1);
	if (total) HIP_TRY(h, hipMemcpyAsync(pk.data(), h->d_str, (size_t)total, hipMemcpyDeviceToHost, s));
	HIP_TRY(h, hipStreamSynchronize(s));
	for (int64_t p = 0; p < npairs; ++p)
		if (out_nops[p] > 0) memcpy(out_ops + ops_off[p], pk.data() + h_poff[(size_t)p], (size_t)out_nops[p]);
	return AT_OK;
}

extern "C" int at_align_allpairs(at_handle *h, int mode, int64_t nreads, const uint8_t *seq_blob,
                                 const int64_t *off, const int32_t *len, int64_t first_pair, int64_t npairs, int want_traceback,
                                 int32_t *out_score, int32_t *out_end_i, int32_t *out_end_j, int32_t *out_state,
                                 uint8_t *out_ops, const int64_t *ops_off, int32_t *out_nops)
{
	int rc = check_allpairs_args(h, "at_align_allpairs", mode, nreads, first_pair, npairs);
	if (rc) return rc;
	if (npairs == 0) return AT_OK;
	if (!seq_blob || !off || !len || !out_score) return fail(h, AT_ERR_ARG, "NULL argument");
	const bool tb = want_traceback && mode != AT_MODE_EDIT;
	if (tb && (!out_ops || !ops_off || !out_nops)) return fail(h, AT_ERR_ARG, "traceback wanted but ops buffers are NULL");
	return guarded(h, "at_align_allpairs", [&] {
		ReadSet rs;
		int rc2 = upload_reads(h, mode, nreads, seq_blob, off, len, &rs);
		if (rc2) return rc2;
		if (!tb) {
			CopyOut co = {first_pair, out_score, out_end_i, out_end_j, out_state};
			return allpairs_scores(h, mode, nreads, rs, first_pair, npairs, 0, copy_out_slice, &co);
		}
		/* with tracebacks: slices whose ops slots (2 * maxlen bytes per pair) stay below ~1 GiB of device memory */
		const int64_t per = std::max<int64_t>(1, std::min<int64_t>(1LL << 22, (1LL << 30) / std::max(1, 2 * rs.maxlen)));
		for (int64_t lo = 0; lo < npairs; lo += per) {
			const int64_t n = std::min(per, npairs - lo);
			rc2 = allpairs_tb_slice(h, mode, nreads, rs, first_pair + lo, n, out_score + lo, out_end_i ? out_end_i + lo : nullptr,
			                        out_end_j ? out_end_j + lo : nullptr, out_state ? out_state + lo : nullptr, out_ops, ops_off + lo, out_nops + lo);
			if (rc2) return rc2;
		}
		return (int)AT_OK;
	});
}

/* ---- all-vs-all of which only the pairs over a threshold leave the device (at_allpairs_hits; the stages: at_pairhits.hip.h) ----
 * The slices, their two buffer sets and their events are those of allpairs_scores; what differs is behind the sweep: the flag, prefix
 * sum and emit kernels on the handle's stream, then 16 bytes (the smallest pair outside the domain, the kept count) on the copy
 * stream, and -- once the host has the count, while the next slice is swept -- the kept records. */
struct PairHitsRun { int64_t nslices = 0, chunk = 0; std::string cfg0; };

static int allpairs_hit_slices(at_handle *h, int mode, int64_t nreads, const ReadSet &rs, int64_t first_pair, int64_t npairs,
                               int64_t chunk, int32_t threshold, std::vector<at::PairHit> &hits, PairHitsRun &run)
{
	if (chunk <= 0) chunk = env_ll("AT_ALLPAIRS_CHUNK", at::kSliceDefault);
	chunk = std::max<int64_t>(1, std::min<int64_t>(chunk, std::min<int64_t>(npairs, at::kSliceMost)));
	int32_t *d_res[2][4]; int *d_flag = nullptr; long long *d_off = nullptr; unsigned long long *d_slots[2]; at::PairHit *d_rec[2];
	int rc = carve(h, &h->d_out, &h->out_bytes, [&](Carver &c) { for (auto &set : d_res) for (int32_t *&x : set) x = c.take<int32_t>((size_t)chunk); });
	/* [flags | prefix sums | 2 x (the two 64-bit slots | the slice's records)] */
	if (!rc) rc = carve(h, &h->d_cand, &h->cand_bytes, [&](Carver &c) {
		d_flag = c.take<int>((size_t)chunk); d_off = c.take<long long>((size_t)chunk + 1);
		for (int q = 0; q < 2; ++q) { d_slots[q] = c.take<unsigned long long>(1); d_rec[q] = c.take<at::PairHit>((size_t)chunk); }
	});
	if (rc) return rc;
	if (h->pin_bytes < 256) {
		if (h->h_pin) { (void)hipHostFree(h->h_pin); h->h_pin = nullptr; h->pin_bytes = 0; }
		if (hipHostMalloc(&h->h_pin, 4096, hipHostMallocDefault) != hipSuccess) {
			h->h_pin = nullptr;
			(void)hipGetLastError();   /* (as in grow) */
			return fail(h, AT_ERR_NOMEM, "hipHostMalloc(%d) for the slices' counts failed", 4096);
		}
		h->pin_bytes = 4096;
	}
	if (!h->copy_stream) HIP_TRY(h, hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
	for (int q = 0; q < 2; ++q) {
		if (!h->ev_sweep[q]) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_sweep[q], hipEventDisableTiming));
		if (!h->ev_copy[q]) HIP_TRY(h, hipEventCreateWithFlags(&h->ev_copy[q], hipEventDisableTiming));
	}
	hipStream_t s = h->stream, cs = h->copy_stream;
	const int64_t nchunks = (npairs + chunk - 1) / chunk;
	auto hslots = [&](int q) { return (volatile unsigned long long *)((char *)h->h_pin + (size_t)q * 64); };
	auto deliver = [&](int64_t c) -> int {
		const int q = (int)(c & 1);
		const int64_t lo = c * chunk, n = std::min(chunk, npairs - lo);
		HIP_TRY(h, hipEventSynchronize(h->ev_copy[q]));
		const unsigned long long bad = hslots(q)[0], kept = hslots(q)[1];
		if (bad != at::kPairHitsNoBad)
			return fail(h, AT_ERR_DOMAIN, "pair %lld: input outside the domain on which the reference is defined", (long long)bad);
		if (kept > (unsigned long long)n) return fail(h, AT_ERR_RANGE, "at_allpairs_hits: %llu hits kept of the %lld pairs from %lld", kept, (long long)n, (long long)(first_pair + lo));
		if (kept > 0) {
			const size_t was = hits.size();
			hits.resize(was + (size_t)kept);
			HIP_TRY(h, hipMemcpyAsync(hits.data() + was, d_rec[q], (size_t)kept * sizeof(at::PairHit), hipMemcpyDeviceToHost, cs));
			HIP_TRY(h, hipStreamSynchronize(cs));
		}
		return AT_OK;
	};
	for (int64_t c = 0; c < nchunks; ++c) {
		const int q = (int)(c & 1);
		const int64_t lo = c * chunk, n = std::min(chunk, npairs - lo);
		/* (slice c - 2, the last user of buffer set q, was delivered before slice c - 1 was queued) */
		BatchReq r = triangle_req(h, mode, rs, nreads, first_pair + lo, n, s);
		r.d_score = d_res[q][0]; r.d_end_i = d_res[q][1]; r.d_end_j = d_res[q][2]; r.d_state = d_res[q][3];
		/* overlap: the bit-parallel bound with this call's threshold, whatever at_set_min_score says */
		if (mode == AT_MODE_OVERLAP) { r.min_on = 1; r.min_score = threshold; }
		rc = align_device(h, r);
		if (rc) { (void)hipDeviceSynchronize(); return rc; }
		if (c == 0) run.cfg0 = h->cfg;
		at::PairHitsArgs pa;
		memset(&pa, 0, sizeof pa);
		pa.n = n; pa.first = first_pair + lo; pa.nreads = nreads;
		pa.score = d_res[q][0]; pa.end_i = d_res[q][1]; pa.end_j = d_res[q][2]; pa.state = d_res[q][3];
		pa.threshold = threshold; pa.is_edit = mode == AT_MODE_EDIT ? 1 : 0;
		pa.flag = d_flag; pa.off = d_off; pa.hits = d_rec[q]; pa.cap = chunk; pa.slots = d_slots[q];
		auto select = [&]() -> int {
			HIP_TRY(h, hipMemsetAsync(d_slots[q], 0xff, 8, s));
			HIP_TRY(h, at_pairhits_flag_launch(&pa, h->ncu, s));
			if (int rcs = scan_nops_device(h, n, d_flag, (int64_t *)d_off, s)) return rcs;
			HIP_TRY(h, at_pairhits_emit_launch(&pa, h->ncu, s));
			HIP_TRY(h, hipEventRecord(h->ev_sweep[q], s));
			return AT_OK;
		};
		rc = select();
		if (rc == AT_OK && c >= 1) rc = deliver(c - 1);
		if (rc) { (void)hipDeviceSynchronize(); return rc; }
		HIP_TRY(h, hipStreamWaitEvent(cs, h->ev_sweep[q], 0));
		HIP_TRY(h, hipMemcpyAsync((void *)hslots(q), d_slots[q], 16, hipMemcpyDeviceToHost, cs));
		HIP_TRY(h, hipEventRecord(h->ev_copy[q], cs));
	}
	rc = deliver(nchunks - 1);
	if (rc) return rc;
	run.nslices = nchunks; run.chunk = chunk;
	return AT_OK;
}

/* the alignments of n hits (one piece): pair list and op slots from the records, the sweep with tracebacks, the runs, the check */
static int pairhits_cigars(at_handle *h, int mode, const ReadSet &rs, const at::PairHit *hits, int64_t n, int64_t ops_bytes, int flags,
                           const CigarOut &co, std::string *tbcfg)
{
	const int64_t dcap = std::min<int64_t>(co.cap, ops_bytes);   /* (a list has no more runs than ops) */
	hipStream_t s = h->stream;
	WindowBufs w;
	int rc = window_carve(h, n, dcap, (size_t)n * sizeof(at::PairHit), false, false, &h->d_str, &h->str_bytes, ((size_t)ops_bytes + 64 + 255) & ~(size_t)255, w);
	if (rc) return rc;
	HIP_TRY(h, hipMemcpyAsync(w.front, hits, (size_t)n * sizeof(at::PairHit), hipMemcpyHostToDevice, s));
	HIP_TRY(h, hipMemsetAsync(w.bad, 0, 4, s));
	at::PairHitsDescArgs da;
	memset(&da, 0, sizeof da);
	da.n = n; da.hits = (const at::PairHit *)w.front; da.swoff = (const long long *)rs.d_swoff; da.slen = rs.d_len;
	da.woff1 = (long long *)w.woff1; da.woff2 = (long long *)w.woff2; da.len1 = w.len1; da.len2 = w.len2; da.nslot = w.aux;
	da.score2 = w.sc; da.end_i2 = w.ei; da.end_j2 = w.ej; da.bad = w.bad;
	HIP_TRY(h, at_pairhits_desc_launch(&da, h->ncu, s));
	rc = scan_nops_device(h, n, w.aux, w.ops_off, s);
	if (!rc) rc = align_device(h, window_req(h, mode, n, rs, w, rs.maxlen, rs.maxlen, s));
	if (rc) { (void)hipStreamSynchronize(s); return rc; }
	if (tbcfg && tbcfg->empty()) *tbcfg = h->cfg;
	rc = at_cigar_batch_device(h, n, rs.d_words, rs.bits, w.woff1, w.woff2, w.ei, w.ej, w.ops, w.ops_off, w.nops, flags, w.ncigar, w.stats, w.coff, w.cigar, dcap, s);
	if (rc) { (void)hipStreamSynchronize(s); return rc; }
	HIP_TRY(h, at_pairhits_check_launch(&da, h->ncu, s));
	rc = window_fetch(h, w, n, "at_allpairs_hits: the traceback pass does not reproduce a hit's score and end cell", co.ncigar, co.stats, co.off);
	if (rc) return rc;
	for (int64_t e = 0; e < n; ++e)
		if (co.ncigar[e] < 0) return fail(h, AT_ERR_DOMAIN, "pair %lld: traceback inconsistent with its sequences", hits[e].pair);
	return window_words(h, w, co.off, n, co.cap, co.words);
}

extern "C" int at_allpairs_hits(at_handle *h, int mode, int64_t nreads,
                                const uint8_t *seq_blob, const int64_t *off, const int32_t *len,
                                int64_t first_pair, int64_t npairs, int32_t threshold, int64_t chunk_pairs, int flags,
                                int64_t hit_cap, int64_t *out_nhits,
                                int64_t *out_pair, int32_t *out_a, int32_t *out_b,
                                int32_t *out_score, int32_t *out_end_i, int32_t *out_end_j, int32_t *out_state,
                                int32_t *out_stats, int32_t *out_ncigar, int64_t *out_cigar_off,
                                uint32_t *out_cigar, int64_t cigar_cap)
{
	const char *who = "at_allpairs_hits";
	int rc = check_allpairs_args(h, who, mode, nreads, first_pair, npairs);
	if (rc || (rc = check_one_gpu(h, who))) return rc;
	if (hit_cap < 0 || cigar_cap < 0) return fail(h, AT_ERR_ARG, "at_allpairs_hits: negative capacity");
	const CigarOut co = {out_stats, out_ncigar, out_cigar_off, out_cigar, cigar_cap};
	if ((rc = check_options(h, who, AT_STRAND_FWD, 0, 0, flags, co, 0, 0))) return rc;   /* (flags and CIGAR outputs) */
	const bool cg = co.any();
	if (cg && mode == AT_MODE_EDIT) return fail(h, AT_ERR_ARG, "at_allpairs_hits: edit has no CIGAR here (alignments of edit distances: at_align_batch_cigar)");
	if (!out_nhits || (npairs > 0 && (!seq_blob || !off || !len)) ||
	    (hit_cap > 0 && (!out_pair || !out_a || !out_b || !out_score || !out_end_i || !out_end_j || !out_state)))
		return fail(h, AT_ERR_ARG, "at_allpairs_hits: NULL argument");
	return guarded(h, "at_allpairs_hits", [&]() -> int {
		*out_nhits = 0;
		PairHitsRun run;
		std::vector<at::PairHit> hits;
		auto config = [&]() {
			snprintf(h->cfg, sizeof h->cfg, "allpairs-hits: threshold=%d, %lld slices of <= %lld pairs, kept=%lld; %.300s", threshold,
			         (long long)run.nslices, (long long)run.chunk, (long long)hits.size(), run.cfg0.empty() ? "none" : run.cfg0.c_str());
		};
		if (npairs == 0) {
			if (cg) out_cigar_off[0] = 0;
			config();
			return (int)AT_OK;
		}
		ReadSet rs;
		int rc2 = upload_reads(h, mode, nreads, seq_blob, off, len, &rs);
		if (rc2) return rc2;
		rc2 = allpairs_hit_slices(h, mode, nreads, rs, first_pair, npairs, chunk_pairs, threshold, hits, run);
		if (rc2) return rc2;
		config();
		const int64_t nh = (int64_t)hits.size();
		*out_nhits = nh;
		if (nh > hit_cap) return (int)AT_OK;               /* the caller comes back with room */
		for (int64_t e = 0; e < nh; ++e) {
			const at::PairHit &x = hits[(size_t)e];
			out_pair[e] = x.pair; out_a[e] = x.a; out_b[e] = x.b;
			out_score[e] = x.score; out_end_i[e] = x.end_i; out_end_j[e] = x.end_j; out_state[e] = x.state;
		}
		if (!cg) return (int)AT_OK;
		out_cigar_off[0] = 0;
		if (nh == 0) return (int)AT_OK;
		/* the traceback pass over the hits, in pieces that keep its descriptor and op buffers moderate */
		std::vector<int64_t> p_off;
		std::string tbcfg;
		for (int64_t a = 0, b; a < nh; a = b) {
			int64_t ops = 0;
			b = at::piece_end(a, nh, 1LL << 20, 1LL << 30, [&](int64_t e) { return (int64_t)len[hits[(size_t)e].a] + len[hits[(size_t)e].b]; }, &ops);
			const int64_t n = b - a, base = out_cigar_off[a];
			p_off.assign((size_t)n + 1, 0);
			const int64_t room = std::max<int64_t>(0, cigar_cap - base);
			const CigarOut piece = {out_stats + a * 8, out_ncigar + a, p_off.data(), room > 0 ? out_cigar + base : nullptr, room};
			rc2 = pairhits_cigars(h, mode, rs, hits.data() + a, n, ops, flags, piece, &tbcfg);
			if (rc2) return rc2;
			for (int64_t e = 1; e <= n; ++e) out_cigar_off[a + e] = base + p_off[(size_t)e];
		}
		config();
		cfg_append(h, "; alignments: %.200s, cigars: %d lanes/pair", tbcfg.c_str(), h->last_cigar_lanes);
		return (int)AT_OK;
	});
}

extern "C" int at_align_batch(at_handle *h, int mode, int64_t npairs, const uint8_t *seq_blob,
                              const int64_t *off1, const int32_t *len1, const int64_t *off2, const int32_t *len2,
                              int want_traceback,
                              int32_t *out_score, int32_t *out_end_i, int32_t *out_end_j, int32_t *out_state,
                              uint8_t *out_ops, const int64_t *ops_off, int32_t *out_nops)
{
	return guarded(h, "at_align_batch", [&] {
		return align_host_mt(h, mode, npairs, seq_blob, off1, len1, off2, len2, want_traceback, out_score, out_end_i, out_end_j,
		                     out_state, out_ops, ops_off, out_nops, nullptr, nullptr);
	});
}

extern "C" int at_align_batch_strings(at_handle *h, int mode, int64_t npairs, const uint8_t *seq_blob,
                                      const int64_t *off1, const int32_t *len1, const int64_t *off2, const int32_t *len2,
                                      int32_t *out_score, int32_t *out_end_i, int32_t *out_end_j, int32_t *out_state,
                                      char *out_r1, char *out_r2, const int64_t *str_off, int32_t *out_len)
{
	if (mode == AT_MODE_EDIT && !(h && h->edit_tb)) return fail(h, AT_ERR_ARG, "edit has no alignment strings (alignment.h:291)");
	if (!out_r1 || !out_r2 || !str_off || !out_len) return fail(h, AT_ERR_ARG, "NULL string buffers");
	return guarded(h, "at_align_batch_strings", [&] {
		return align_host_mt(h, mode, npairs, seq_blob, off1, len1, off2, len2, 1, out_score, out_end_i, out_end_j, out_state,
		                     nullptr, str_off, out_len, out_r1, out_r2);
	});
}

extern "C" int at_align_batch_cigar(at_handle *h, int mode, int64_t npairs, const uint8_t *seq_blob,
                                    const int64_t *off1, const int32_t *len1, const int64_t *off2, const int32_t *len2,
                                    int flags,
                                    int32_t *out_score, int32_t *out_end_i, int32_t *out_end_j, int32_t *out_state,
                                    int32_t *out_stats, int32_t *out_ncigar, int64_t *out_cigar_off,
                                    uint32_t *out_cigar, int64_t cigar_cap)
{
	if (!h) return fail(nullptr, AT_ERR_ARG, "at_align_batch_cigar: NULL handle");
	if (mode == AT_MODE_EDIT && !h->edit_tb) return fail(h, AT_ERR_ARG, "edit has no alignment, hence no CIGAR (alignment.h:291)");
	if (npairs < 0 || cigar_cap < 0) return fail(h, AT_ERR_ARG, "negative size");
	if (!out_stats || !out_ncigar || !out_cigar_off || (!out_cigar && cigar_cap > 0)) return fail(h, AT_ERR_ARG, "NULL CIGAR buffers");
	if (npairs == 0) { out_cigar_off[0] = 0; return AT_OK; }
	if (!seq_blob || !off1 || !len1 || !off2 || !len2 || !out_score) return fail(h, AT_ERR_ARG, "NULL argument");
	return guarded(h, "at_align_batch_cigar", [&] {
		/* the op codes stay on the device, in slots of len1 + len2 bytes laid back to back */
		std::vector<int64_t> slot((size_t)npairs);
		std::vector<int32_t> nops((size_t)npairs);
		int64_t at = 0;
		for (int64_t k = 0; k < npairs; ++k) { slot[(size_t)k] = at; at += (int64_t)std::max(len1[k], 0) + std::max(len2[k], 0); }
		CigarReq cg;
		cg.flags = flags; cg.out_stats = out_stats; cg.out_ncigar = out_ncigar; cg.out_off = out_cigar_off;
		return align_host_mt(h, mode, npairs, seq_blob, off1, len1, off2, len2, 1, out_score, out_end_i, out_end_j, out_state,
		                     nullptr, slot.data(), nops.data(), nullptr, nullptr, &cg, out_cigar, cigar_cap);
	});
}
