// The page-warp driver behind ma_warp_pages_host, ma_warp_pages_host_interp and
// ma_warp_affine_flow_pages_host.  Host code only: no kernel lives here.
//
// warp_and_save_pages (microaligner/__main__.py:288-302): every channel / z page of a cycle is warped with the SAME flow.
// The flow stays in HBM; pages stream through NS slots (a device buffer pair each) on the three engines of the context, so
// the upload of one piece, the kernel of the previous one and the download of the one before overlap.  The unit of the
// pipeline is a BAND of output rows, not a page: a single page (Warper.warp() of a host image, the reference's own per-page
// loop) overlaps its own kernels and download -- and, where the caller can bound the source rows a band reads (the tiled
// warps: MaPagePlan::cuts_src), its own upload -- and the first and last page of a longer run lose only a band to filling
// and draining.
#include "ma_internal.h"

#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

// An upload thread copies piece after piece of page i into input slot i % NS on the H2D stream, this thread launches each
// band's warp on the ctx stream once the piece it needs is in, a download thread copies the band's rows out on the D2H
// stream; events order the streams, counters under one mutex order the threads.  Pageable pages (numpy arrays, rows of a
// memmapped TIFF) are staged by the engines through page-locked chunks -- the runtime's own staging of pageable memory
// reached 14 GB/s per direction here, the engines 2 - 3 x that (profiles/r04_notes.md).
int ma_warp_pages_run(ma_ctx* ctx, const void* const* pages_host, void* const* out_host, int n_pages, const MaPagePlan& p,
                      const MaBandFn& launch)
{
    constexpr int NS = 3;
    const int ns = n_pages < NS ? n_pages : NS;
    const int nup = (int)p.cuts_src.size(), nband = (int)p.cuts_out.size();
    MA_REQUIRE(n_pages > 0 && nband > 0 && (nup == nband || nup == 1), "bad page plan");
    // rows of band b, and the upload piece that must be resident before it runs
    auto band_begin = [&](int b) { return (int)((b ? p.cuts_out[b - 1] : 0) / p.out_row_bytes); };
    auto band_end = [&](int b) { return (int)(p.cuts_out[b] / p.out_row_bytes); };
    auto needs = [&](int b) { return nup == 1 ? 0 : b; };
    const size_t in_bytes = ma_align_up(p.in_bytes, 256), out_bytes = ma_align_up(p.out_bytes, 256);
    MA_TRY(ma_ws_reserve(ctx, (in_bytes + out_bytes) * ns));  // device buffers come from the context workspace
    char *din[NS], *dout[NS];
    for (int k = 0; k < ns; k++) {
        din[k] = (char*)ctx->ws + (in_bytes + out_bytes) * k;
        dout[k] = din[k] + in_bytes;
    }
    // The slots live in the context workspace, which kernels enqueued earlier on the compute stream (a tiled Farneback,
    // a dog(), the NMI) may still be using: both transfer engines start behind everything the compute stream holds now
    // (ma_ws_reserve itself synchronises only when the workspace has to grow).
    {
        hipEvent_t ws_idle = ma_ctx_sync_event(ctx, MA_EV_WARP_PAGES);
        hipStream_t s_up = ma_engine_stream(ctx, MA_ENGINE_H2D), s_down = ma_engine_stream(ctx, MA_ENGINE_D2H);
        if (!ws_idle || !s_up || !s_down) return MA_EHIP;
        MA_HIP(hipEventRecord(ws_idle, ctx->stream));
        MA_HIP(hipStreamWaitEvent(s_up, ws_idle, 0));
        MA_HIP(hipStreamWaitEvent(s_down, ws_idle, 0));
    }
    std::vector<hipEvent_t> ev_up((size_t)ns * nup, nullptr), ev_k((size_t)ns * nband, nullptr);
    auto cleanup = [&]() {
        for (hipEvent_t e : ev_up) if (e) (void)hipEventDestroy(e);
        for (hipEvent_t e : ev_k) if (e) (void)hipEventDestroy(e);
    };
    for (std::vector<hipEvent_t>* evs : {&ev_up, &ev_k})
        for (hipEvent_t& e : *evs)
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
                cleanup();
                ma_set_error("hipEventCreate failed");
                return MA_EHIP;
            }
    const bool TRACE = getenv("MICROALIGNER_TRACE_PAGES") != nullptr;   // timeline of the three threads on stderr
    const auto T0 = std::chrono::steady_clock::now();
    auto now_ms = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - T0).count(); };
    if (TRACE) fprintf(stderr, "[pages] %d pages, %d bands of %d rows\n", n_pages, nband, band_end(0));
    std::mutex mu;
    std::condition_variable cv;
    long long uploaded = 0, launched = 0;   // in units: (page * nup + piece), (page * nband + band)
    int downloaded = 0;                     // in pages
    int failed = MA_OK;
    std::string what;
    auto fail = [&](int rc) {   // called with mu held, on the thread whose ma_last_error() explains rc
        if (failed == MA_OK) { failed = rc; what = ma_last_error(); }
        cv.notify_all();
    };
    // A page is ONE copy per direction (ma_engine_*_pieces): the staging of pageable memory keeps its chunks in flight
    // across the piece boundaries, the pieces only decide when the events are recorded and waited for.
    std::thread up([&]() {
        for (int i = 0; i < n_pages; i++) {
            const int k = i % ns;
            {   // slot k, input and output half, is free again once page i - ns has been downloaded
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return failed != MA_OK || downloaded > i - ns; });
                if (failed != MA_OK) return;
            }
            const int rc = ma_engine_h2d_pieces(ctx, MA_ENGINE_H2D, din[k], pages_host[i], p.in_bytes, p.cuts_src.data(), nup, [&](int j) {
                const int r = ma_engine_record(ctx, MA_ENGINE_H2D, ev_up[(size_t)k * nup + j]);
                if (TRACE) fprintf(stderr, "[pages] %8.2f up   p%d b%d\n", now_ms(), i, j);
                std::lock_guard<std::mutex> lk(mu);
                if (r != MA_OK) return r;
                if (failed != MA_OK) return failed;
                uploaded = (long long)i * nup + j + 1;
                cv.notify_all();
                return (int)MA_OK;
            }, false);   // no wait at the page boundary: the next page's first chunk is staged under this page's last DMAs
            if (rc != MA_OK) {
                std::lock_guard<std::mutex> lk(mu);
                fail(rc);
                return;
            }
        }
        const int rc = ma_engine_sync(ctx, MA_ENGINE_H2D);
        if (rc != MA_OK) {
            std::lock_guard<std::mutex> lk(mu);
            fail(rc);
        }
    });
    std::thread down([&]() {
        for (int i = 0; i < n_pages; i++) {
            const int k = i % ns;
            const int rc = ma_engine_d2h_pieces(ctx, MA_ENGINE_D2H, out_host[i], dout[k], p.out_bytes, p.cuts_out.data(), nband, [&](int b) {
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [&] { return failed != MA_OK || launched > (long long)i * nband + b; });
                    if (failed != MA_OK) return failed;
                }
                if (TRACE) fprintf(stderr, "[pages] %8.2f down p%d b%d (issued)\n", now_ms(), i, b);
                return ma_engine_wait(ctx, MA_ENGINE_D2H, ev_k[(size_t)k * nband + b]);
            });
            std::lock_guard<std::mutex> lk(mu);
            if (rc != MA_OK) { fail(rc); return; }
            if (TRACE) fprintf(stderr, "[pages] %8.2f down p%d complete\n", now_ms(), i);
            downloaded = i + 1;
            cv.notify_all();
        }
    });
    const long long n_units = (long long)n_pages * nband;
    for (long long u = 0; u < n_units; u++) {
        const int i = (int)(u / nband), b = (int)(u % nband), k = i % ns;
        {
            std::unique_lock<std::mutex> lk(mu);
            cv.wait(lk, [&] { return failed != MA_OK || uploaded > (long long)i * nup + needs(b); });
            if (failed != MA_OK) break;
        }
        const int y0 = band_begin(b), y1 = band_end(b);
        int rc = MA_OK;
        // (a page that went up whole: its one upload event orders every band once it orders the first)
        if (b == 0 || nup > 1) rc = ma_engine_wait(ctx, MA_ENGINE_COMPUTE, ev_up[(size_t)k * nup + needs(b)]);
        if (rc == MA_OK) rc = launch(din[k], dout[k], y0, y1);
        if (rc == MA_OK) rc = ma_engine_record(ctx, MA_ENGINE_COMPUTE, ev_k[(size_t)k * nband + b]);
        if (TRACE) fprintf(stderr, "[pages] %8.2f kern p%d b%d\n", now_ms(), i, b);
        std::lock_guard<std::mutex> lk(mu);
        if (rc != MA_OK) {
            const std::string why = ma_last_error();
            ma_set_error("warp of page %d (rows %d..%d) failed: %s", i, y0, y1, why.c_str());
            fail(rc);
            break;
        }
        launched = u + 1;
        cv.notify_all();
    }
    up.join();
    down.join();
    if (TRACE) fprintf(stderr, "[pages] %8.2f joined\n", now_ms());
    // also when a thread gave up early: nothing of this call may still be reading the caller's pages or writing its
    // results once it has returned
    (void)ma_engine_sync(ctx, MA_ENGINE_H2D);
    (void)ma_engine_sync(ctx, MA_ENGINE_D2H);
    (void)hipStreamSynchronize(ctx->stream);
    cleanup();
    if (TRACE) fprintf(stderr, "[pages] %8.2f cleaned\n", now_ms());
    if (failed != MA_OK) {
        ma_set_error("%s", what.c_str());
        return failed;
    }
    return MA_OK;
}
