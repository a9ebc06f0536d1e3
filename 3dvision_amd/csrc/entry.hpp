// The frame of a public call (included by tdv_internal.hpp): what every extern "C" entry point does around its stage.  The rule that a
// call's outputs depend on its arguments and the ctx's settings only (tests/test_gpu_ctx_state.py) starts here: call_begin is the one
// place outside ctx.hip and the batch lanes' helper contexts where a ctx's device is selected and its workspace reset.
#pragma once
#include <initializer_list>

namespace tdv {

// TDV_ERR_BAD_ARG for a NULL ctx; selects the ctx's device and clears its error text.  Touches nothing else: an entry point that can
// still refuse the call (tdv_register_batch_dev's loss check, comm.hip's root check) does so between this and ws_reset, which may wait
// on the stream and reallocate when it coalesces blocks.
int call_enter(tdv_ctx* ctx);
// call_enter, then ws_reset: the prologue of every other entry point, after its argument checks
int call_begin(tdv_ctx* ctx);

// host array -> fresh workspace memory, enqueued on the ctx stream (*dev = nullptr for a NULL or empty array)
template <class T>
int upload(tdv_ctx* ctx, const T* host, size_t count, T** dev) {
    *dev = nullptr;
    if (!host || count == 0) return TDV_OK;
    TDV_TRY(ws_alloc(ctx, count, dev));
    TDV_HIP(ctx, hipMemcpyAsync(*dev, host, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    return TDV_OK;
}
// device -> host array, enqueued (nothing for a NULL pointer on either side)
template <class T>
int download(tdv_ctx* ctx, T* host, const T* dev, size_t count) {
    if (!host || !dev || count == 0) return TDV_OK;
    TDV_HIP(ctx, hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    return TDV_OK;
}
inline int finish(tdv_ctx* ctx) {
    TDV_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return TDV_OK;
}

// A call's state record: device -> the pinned block (the caller has done pin_reserve for at least sizeof(T)), one wait, then *out.
// Downloads the caller enqueued before ride the same wait.
template <class T>
int fetch_state(tdv_ctx* ctx, const T* d_state, T* out) {
    TDV_HIP(ctx, hipMemcpyAsync(ctx->pin, d_state, sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    TDV_TRY(finish(ctx));
    std::memcpy(out, ctx->pin, sizeof(T));
    return TDV_OK;
}

// The leading m rows of every pair whose two pointers are non-NULL, device -> host, and one wait if anything was copied: the rows a
// call kept, once the state record has said how many (the device arrays hold nothing beyond).  m == 0 does nothing.
struct RowCopy { void* host; const void* dev; size_t row_bytes; };
int download_rows(tdv_ctx* ctx, size_t m, std::initializer_list<RowCopy> rows);

}  // namespace tdv
