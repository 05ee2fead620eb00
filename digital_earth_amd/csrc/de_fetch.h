// de_fetch.h — how an output leaves the GPU, each mechanism stated once (the state they work on is in de_context.h: FetchRing, PackedOut; the buffers
// "of at least n bytes" they are made of are de_memory.h's Pinned and Dev):
//   * the ring arithmetic of the lagged fetches, plain integers;
//   * copy_out: device -> caller's buffer through the context's staging buffer;
//   * the conversion frame of the packed outputs (8-bit pixels, HDR pixels, video frames): allocate, display, phase, launch, count;
//   * the synchronous path (render, copy, wait) and the lagged one (begin: render, copy, record; end: wait, hand out);
//   * both once more for the outputs whose length the device decides (CodedOut: the JPEG stream, the PNG, OpenEXR and Radiance files);
//   * the entry points of those outputs, once over a format's descriptor (coded_capacity ... coded_fetch_end), and the one frame of their debug
//     conversions (coded_debug).
// The entry points of de_api.hip check their own arguments and call one of these.
#pragma once

// ---- ring arithmetic.  No HIP: tools/fetch_ring_host_check.cpp compiles this part alone (DE_FETCH_STANDALONE) under the address and undefined-behaviour
// sanitizers.  `begun` and `ended` count the calls of _begin and _end and wrap at 2^32, a multiple of the depth (a power of two): across the wrap their
// difference is still the number of fetches in flight, and each of them modulo the depth still visits the cells in the one order 0, 1, .., depth - 1, 0, ..
inline unsigned ring_in_flight(unsigned begun, unsigned ended) { return begun - ended; }
inline bool ring_full(unsigned begun, unsigned ended, unsigned depth) { return begun - ended >= depth; }      // _begin refuses
inline bool ring_empty(unsigned begun, unsigned ended) { return begun == ended; }                            // _end refuses
inline int ring_cell(unsigned calls, unsigned depth) { return (int)(calls % depth); }                        // of `begun`: the cell _begin fills; of `ended`: the cell _end hands out

#ifndef DE_FETCH_STANDALONE
#include "de_launch.h"

namespace {
static_assert((DE_FETCH_RING & (DE_FETCH_RING - 1)) == 0, "the ring's depth must divide 2^32 (ring arithmetic above)");

// device (W*H*3 floats, or `bytes`) -> caller's buffer through the pinned staging buffer; straight into the caller's pageable memory when none can be had
int copy_out(de_ctx* c, float* out, const float* d_src, size_t bytes = 0) {
    if (!bytes) bytes = (size_t)c->W * c->H * 3 * sizeof(float);
    const bool staged = c->h_stage.ensure(bytes) == hipSuccess;      // (no copy into it is in flight: every staged copy is waited for before its call returns)
    HIP_TRY(hipMemcpyAsync(staged ? c->h_stage.get() : out, d_src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (staged) memcpy(out, c->h_stage, bytes);
    return frame_status(c);
}

// ---- the packed outputs.  One conversion: the displayed image, then `launch(phase)` packs it into o.dev.  de_render_to_image records ev_main behind the
// display and ahead of everything enqueued here and by the fetches below — the pack, the copy — so the next frame's sums wait for neither.  The dither
// phase is the number of conversions since the settings were set while they animate, 0 otherwise.
template <class Launch>
int render_packed(de_ctx* c, PackedOut& o, size_t capacity, bool animate, Launch launch) {
    HIP_TRY(hipSetDevice(c->device));
    int rc = o.dev.ensure(capacity, std::string(o.noun) + " buffers");      // one that is too small is replaced: hipFree waits for the work that reads it
    if (rc) return rc;
    rc = de_render_to_image(c, nullptr);
    if (rc) return rc;
    const uint32_t phase = animate ? o.count : 0u;
    launch(phase);
    HIP_TRY(hipGetLastError());
    o.count++; o.last_phase = phase;
    return DE_OK;
}
void packed_reset(PackedOut& o) { o.count = 0; o.last_phase = 0; }      // new settings

// ---- the synchronous path.  `render` is an output's de_render_to_* entry point: it enqueues the frame as it stands and answers where on the device it
// lies.  `size` bytes of it are copied into `stage`, which holds `capacity` (the largest format: a change of format re-allocates nothing), and waited for.
template <class T, class H>
int fetch_staged(de_ctx* c, Pinned<void>& stage, const char* noun, int (*render)(de_ctx*, const T**), size_t capacity, size_t size, const H** host) {
    HIP_TRY(hipSetDevice(c->device));
    int rc = stage.ensure(capacity, std::string(noun) + " staging buffer");
    if (rc) return rc;
    const T* src = nullptr;
    rc = render(c, &src);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(stage, src, size, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *host = (const H*)stage.get();
    return frame_status(c);
}

// ---- the lagged path (include/digital_earth.h: the window loop pipelined).  begin: the frame as it stands and its copy into the ring's next cell are
// ENQUEUED on the context stream (which waits, on the device, for the launches issued so far); the host returns at once and may issue the next frame's
// de_accumulate — its render launch runs beside the display, the pack and the copy.  end: wait for the oldest fetch begun and hand out its cell.
unsigned in_flight(const FetchRing& r) { return ring_in_flight(r.begun, r.ended); }
int refuse_in_flight(const FetchRing& r) {      // what changes the size or the format of a ring's cells waits for them
    if (in_flight(r)) return fail(DE_ERR_STATE, std::string(r.noun) + " fetches are in flight: " + r.entry + "_end first");
    return DE_OK;
}
int ring_next_cell(const FetchRing& r) { return ring_cell(r.begun, DE_FETCH_RING); }      // the cell the next _begin fills
template <class Pred>
bool ring_any_in_flight(const FetchRing& r, Pred pred) {      // pred(cell) of any fetch begun and not ended, oldest first
    for (unsigned n = r.ended; n != r.begun; ++n) if (pred(ring_cell(n, DE_FETCH_RING))) return true;
    return false;
}
template <class T>
int ring_begin(de_ctx* c, FetchRing& r, int (*render)(de_ctx*, const T**), size_t capacity, size_t size) {
    if (ring_full(r.begun, r.ended, DE_FETCH_RING)) return fail(DE_ERR_STATE, std::string("four ") + r.noun + " fetches are in flight already: " + r.entry + "_end first");
    const int k = ring_cell(r.begun, DE_FETCH_RING);
    HIP_TRY(hipSetDevice(c->device));
    int rc = r.cell[k].ensure(capacity, std::string(r.noun) + " ring");      // cell k is not in flight
    if (rc) return rc;
    if (!r.ev[k]) HIP_TRY(hipEventCreateWithFlags(&r.ev[k], hipEventDisableTiming));
    const T* src = nullptr;
    rc = render(c, &src);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(r.cell[k], src, size, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipEventRecord(r.ev[k], c->stream));
    r.begun++;
    return DE_OK;
}
template <class H>
int ring_end(de_ctx* c, FetchRing& r, const H** host) {
    if (ring_empty(r.begun, r.ended)) return fail(DE_ERR_STATE, std::string("no ") + r.noun + " fetch in flight: " + r.entry + "_begin first");
    const int k = ring_cell(r.ended, DE_FETCH_RING);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(r.ev[k]));
    r.ended++;
    *host = (const H*)r.cell[k].get();
    return frame_status(c);
}
// ---- the same two paths for an output whose length the DEVICE decides (the coded outputs below): on the device it is preceded
// by a `word`-byte header that `length(header, &len)` reads.  A fetch copies the header and then exactly the stream — never the buffer's capacity.
// Synchronous: the header, a wait, the stream, a wait; the staging buffer grows to the longest frame fetched, in steps of 1 MiB.
template <class Length>
int fetch_staged_sized(de_ctx* c, Pinned<void>& stage, const char* noun, const uint8_t* src, size_t word, Length length, const void** host, uint64_t* len) {
    int rc = stage.ensure(word + 4096, std::string(noun) + " staging buffer");
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(stage, src, word, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    rc = frame_status(c);
    if (!rc) rc = length(stage.get(), len);
    if (rc) return rc;
    rc = stage.ensure((word + (size_t)*len + ((size_t)1 << 20) - 1) & ~(((size_t)1 << 20) - 1), std::string(noun) + " staging buffer");
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(stage, src, word + (size_t)*len, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *host = (const uint8_t*)stage.get() + word;
    return DE_OK;
}
// Lagged: _begin cannot know the length without waiting, so it copies a PREFIX of `prefix` bytes (header included) of the stream `render(k)` enqueued
// for cell k — each cell has a device stream of its own, which the next _begin does not touch; _end waits, reads the length and, only if the frame is
// longer than the prefix, copies all of it from that cell's device stream (a wait for what has been enqueued since: the caller sizes the next prefix
// from the lengths it sees, so a steady sequence never comes here).
template <class Render>
int ring_begin_prefix(de_ctx* c, FetchRing& r, Render render, size_t prefix, size_t* copied) {
    if (ring_full(r.begun, r.ended, DE_FETCH_RING)) return fail(DE_ERR_STATE, std::string("four ") + r.noun + " fetches are in flight already: " + r.entry + "_end first");
    const int k = ring_cell(r.begun, DE_FETCH_RING);
    HIP_TRY(hipSetDevice(c->device));
    int rc = r.cell[k].ensure(prefix, std::string(r.noun) + " ring");      // cell k is not in flight
    if (rc) return rc;
    if (!r.ev[k]) HIP_TRY(hipEventCreateWithFlags(&r.ev[k], hipEventDisableTiming));
    const uint8_t* src = nullptr;
    rc = render(k, &src);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(r.cell[k], src, prefix, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipEventRecord(r.ev[k], c->stream));
    copied[k] = prefix;
    r.begun++;
    return DE_OK;
}
template <class Source, class Length>
int ring_end_sized(de_ctx* c, FetchRing& r, Source source, const size_t* copied, size_t word, Length length, const void** host, uint64_t* len) {
    if (ring_empty(r.begun, r.ended)) return fail(DE_ERR_STATE, std::string("no ") + r.noun + " fetch in flight: " + r.entry + "_begin first");
    const int k = ring_cell(r.ended, DE_FETCH_RING);
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(r.ev[k]));
    r.ended++;
    int rc = frame_status(c);
    if (!rc) rc = length(r.cell[k].get(), len);
    if (rc) return rc;
    if (word + (size_t)*len > copied[k]) {
        rc = r.cell[k].ensure((word + (size_t)*len + 4095) & ~(size_t)4095, std::string(r.noun) + " ring");
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(r.cell[k], source(k), word + (size_t)*len, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    *host = (const uint8_t*)r.cell[k].get() + word;
    return DE_OK;
}
// ---- the coded outputs (CodedOut; the word and the failure rule: coded_stream.h).  An output brings its `length` — coded_read_word
// with its two messages —, its render function, its first estimate, its capacity and its refusal texts; everything else is here.
size_t coded_stream_bytes(size_t capacity) { return (CS_WORD_BYTES + capacity + 15) & ~(size_t)15; }      // a stream of that capacity on the device
int coded_read_word(const void* word, uint64_t* len, const char* overflow, const char* range) {      // the length, or DE_ERR_INTERNAL with the status' message
    uint32_t status;
    cs_word_fields(word, len, &status);
    if (status) return fail(DE_ERR_INTERNAL, status & CS_STATUS_OVERFLOW ? overflow : range);
    return DE_OK;
}
template <class Length>      // the stream an output's de_render_to_* has just enqueued into o.out.dev
int coded_view(de_ctx* c, CodedOut& o, Length length, const void** host, uint64_t* len) {
    return fetch_staged_sized(c, o.out.stage, o.out.noun, o.out.dev, CS_WORD_BYTES, length, host, len);
}
int coded_copy_out(const void* host, uint64_t len, void* out, uint64_t out_bytes, const char* refusal) {
    if (out_bytes < len) return fail(DE_ERR_INVALID, refusal);
    memcpy(out, host, (size_t)len);
    return DE_OK;
}
// begin: `first` bytes of stream are the estimate while no frame has ended; render(k) converts the frame as it stands into o.cell[k].
template <class Render>
int coded_begin(de_ctx* c, CodedOut& o, size_t first, size_t capacity, Render render) {
    size_t prefix = o.guess ? o.guess : CS_WORD_BYTES + first;
    if (prefix > CS_WORD_BYTES + capacity) prefix = CS_WORD_BYTES + capacity;
    return ring_begin_prefix(c, o.ring, [&](int k, const uint8_t** src) { int rc = render(k); *src = o.cell[k]; return rc; }, prefix, o.copied);
}
template <class Length>
int coded_end(de_ctx* c, CodedOut& o, Length length, const void** host, uint64_t* len) {
    int rc = ring_end_sized(c, o.ring, [&o](int k) { return (const uint8_t*)o.cell[k].get(); }, o.copied, CS_WORD_BYTES, length, host, len);
    if (!rc) o.guess = ((CS_WORD_BYTES + (size_t)*len) * 5 / 4 + 4095) & ~(size_t)4095;      // the next prefix: a quarter more than this frame
    return rc;
}
// The tail of a debug conversion that has just been launched into d_out on `stream`: the word, the refusal of too small an `out`, the stream itself.
template <class Length>
int coded_debug_out(hipStream_t stream, const uint8_t* d_out, Length length, void* out, uint64_t out_bytes, uint64_t* len, const char* refusal) {
    HIP_TRY(hipGetLastError());
    uint32_t word[CS_WORD_BYTES / 4];
    HIP_TRY(hipMemcpyAsync(word, d_out, sizeof(word), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    { int rc = length(word, len); if (rc) return rc; }
    if (out_bytes < *len) return fail(DE_ERR_INVALID, refusal);
    HIP_TRY(hipMemcpyAsync(out, d_out + CS_WORD_BYTES, (size_t)*len, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    return DE_OK;
}
// A debug conversion on host-given data, once: the device, the stream's buffer, `body(stream, d_out)` — the format's buffers, its uploads
// (debug_upload) and its launches — and the tail above.  The rule: from the body's first upload on a copy that reads the caller's memory may be in
// flight, so every way out behind that point waits for the stream.  `wait`, and nothing else, sees to it; what the copies read and write outlives
// it: the body's device buffers and host arrays are the caller's locals, declared outside the body.
struct StreamWait { hipStream_t stream; ~StreamWait() { (void)hipStreamSynchronize(stream); } };
template <class T>
int debug_upload(hipStream_t stream, Dev<T>& d, const void* host, size_t bytes) {
    HIP_TRY(d.ensure(bytes));
    HIP_TRY(hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, stream));
    return DE_OK;
}
template <class Length, class Body>
int coded_debug(de_ctx* c, size_t capacity, Length length, void* out, uint64_t out_bytes, uint64_t* len, const char* refusal, Body body) {
    HIP_TRY(hipSetDevice(c->device));
    Dev<uint8_t> d_out;
    HIP_TRY(d_out.ensure(coded_stream_bytes(capacity)));
    StreamWait wait{c->stream};
    { int rc = body(c->stream, d_out.get()); if (rc) return rc; }
    return coded_debug_out(c->stream, d_out, length, out, out_bytes, len, refusal);
}
// ---- the entry points of a coded output, once.  A format is a descriptor D (de_display.h: JpegOut, PngOut, ExrOut, RgbeOut) that supplies what differs:
//   coded(c)                 its CodedOut in the context
//   size_refusal(c)          what makes its geometry meaningless: all de_*_capacity refuses
//   refusal(c)               what de_render_to_* and de_fetch_*_begin refuse ahead of everything, size_refusal last
//   geometry(c)              of the frame as it stands: .capacity bounds every stream;  first_prefix(g): what the first _begin copies
//   render(c, dev, k)        one conversion into `dev`, the stream of ring cell k or (k < 0) of the synchronous fetches; behind refusal(c)
//   reads_panorama(c)        whether that conversion reads what de_set_panorama replaces (CodedOut::reads_pano)
//   length(word, &len)       coded_read_word with its messages;  too_small: de_fetch_*'s refusal of a short `out`
// A fifth format writes its descriptor and six one-line entry points.
template <class D>
int coded_capacity(de_ctx* c, uint64_t* bytes) {
    if (!c || !bytes) return fail(DE_ERR_INVALID, "null argument");
    { int rc = D::size_refusal(c); if (rc) return rc; }
    *bytes = (uint64_t)D::geometry(c).capacity;
    return DE_OK;
}
template <class D>
int coded_render_to(de_ctx* c, const void** device_stream, const uint64_t** device_len) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    { int rc = D::refusal(c); if (rc) return rc; }
    Dev<uint8_t>& dev = D::coded(c).out.dev;
    int rc = D::render(c, dev, -1);
    if (rc) return rc;
    if (device_stream) *device_stream = dev + CS_WORD_BYTES;
    if (device_len) *device_len = reinterpret_cast<const uint64_t*>(dev.get());
    return DE_OK;
}
template <class D>
int coded_fetch_view(de_ctx* c, const void** host, uint64_t* len) {
    if (!c || !host || !len) return fail(DE_ERR_INVALID, "null argument");
    int rc = coded_render_to<D>(c, nullptr, nullptr);
    if (rc) return rc;
    return coded_view(c, D::coded(c), D::length, host, len);
}
template <class D>
int coded_fetch(de_ctx* c, void* out, uint64_t out_bytes, uint64_t* len) {
    if (!c || !out || !len) return fail(DE_ERR_INVALID, "null argument");
    const void* host = nullptr;
    int rc = coded_fetch_view<D>(c, &host, len);
    if (rc) return rc;
    return coded_copy_out(host, *len, out, out_bytes, D::too_small);
}
template <class D>
int coded_fetch_begin(de_ctx* c) {
    if (!c) return fail(DE_ERR_INVALID, "null context");
    { int rc = D::refusal(c); if (rc) return rc; }
    CodedOut& o = D::coded(c);
    const auto g = D::geometry(c);
    const int cell = ring_next_cell(o.ring);
    int rc = coded_begin(c, o, D::first_prefix(g), g.capacity, [c, &o](int k) { return D::render(c, o.cell[k], k); });
    if (!rc) o.reads_pano[cell] = D::reads_panorama(c);      // de_set_panorama waits for it
    return rc;
}
template <class D>
int coded_fetch_end(de_ctx* c, const void** host, uint64_t* len) {
    if (!c || !host || !len) return fail(DE_ERR_INVALID, "null argument");
    return coded_end(c, D::coded(c), D::length, host, len);
}
// what changes the panorama's buffers waits for the lagged fetches that read them
int refuse_panorama_readers(const CodedOut& o) {
    if (ring_any_in_flight(o.ring, [&o](int k) { return o.reads_pano[k]; })) return refuse_in_flight(o.ring);
    return DE_OK;
}
void coded_reset(CodedOut& o) { o.guess = 0; packed_reset(o.out); }      // new settings: the first estimate again
void ring_destroy_events(FetchRing& r) {      // de_destroy; the cells free themselves
    for (hipEvent_t& ev : r.ev) { if (ev) hipEventDestroy(ev); ev = nullptr; }
}

}  // namespace
#endif  // DE_FETCH_STANDALONE
