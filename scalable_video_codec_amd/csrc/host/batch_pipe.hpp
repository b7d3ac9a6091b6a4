// batch_pipe.hpp -- the three-stream batch schedule of svc::StreamEncoder and svc::StreamDecoder: H2D on one stream, kernels on a
// second, D2H on a third, `depth` batch slots in a ring, results delivered in order.
//
// The rule both public headers state follows from the two numbers here: batch k uses slot k % depth, and the oldest batch is
// delivered once depth - 1 are pending -- so what a delivery hands out stays untouched until depth - 2 more have been delivered, and
// a setting read while batch j + depth - 1 is staged is the first one that can follow the delivery of batch j.
//
// The pipe owns the streams, the events and the bookkeeping; the caller keeps its buffers per slot, in an array of its own indexed
// by the slot number the pipe hands out, and says what a batch does on each stream:
//
//   pipe.Begin(deliver);                    // deliver(slot): the batch in `slot` has landed in host memory
//   while (more) {
//     const uint32_t slot = pipe.Acquire(); // free to rewrite: whatever used it last has left the device
//     ... stage the batch into the slot's pinned buffers (or find that there is none: Acquire alone commits to nothing) ...
//     pipe.Submit(slot, h2d, kernels, d2h); // each gets its stream; h2d and d2h return the bytes they move
//   }
//   const BatchPipe::Totals& t = pipe.Finish();
#pragma once

#include <chrono>
#include <functional>
#include <vector>

#include "hip_raii.hpp"

namespace svc {
namespace host __attribute__((visibility("hidden"))) {

class BatchPipe {
 public:
  struct Totals {  // of one Begin .. Finish
    uint32_t batches = 0;
    double wall_ms = 0;
    double slot_wait_ms = 0;     // host: inside Acquire, waiting for a slot whose previous results are still on their way back
    double deliver_wait_ms = 0;  // host: waiting for a batch's results before handing it to deliver
    double h2d_ms = 0, kernels_ms = 0, d2h_ms = 0;  // device, per stream
    uint64_t h2d_bytes = 0, d2h_bytes = 0;
  };
  using Deliver = std::function<void(uint32_t slot)>;

  BatchPipe(const Who& who, uint32_t depth) : who_(who), s_in_(who), s_compute_(who), s_out_(who) {
    for (uint32_t i = 0; i < depth; ++i) slots_.emplace_back(who);
  }

  // before buffers that batches in flight may use are resized
  void SyncStreams() {
    for (hipStream_t s : {(hipStream_t)s_in_, (hipStream_t)s_compute_, (hipStream_t)s_out_}) who_.Hip(hipStreamSynchronize(s), "hipStreamSynchronize");
  }

  void Begin(Deliver deliver) {
    deliver_ = std::move(deliver);
    next_ = delivered_ = 0;
    totals_ = Totals{};
    t_begin_ = Clock::now();
  }

  uint32_t Acquire() {
    const uint32_t slot = next_ % (uint32_t)slots_.size();
    Slot& s = slots_[slot];
    if (s.busy) {
      const Clock::time_point t0 = Clock::now();
      who_.Hip(hipEventSynchronize(s.d2h_done), "hipEventSynchronize");
      totals_.slot_wait_ms += MsSince(t0);
      s.busy = false;
    }
    return slot;
  }

  template <typename H2D, typename Kernels, typename D2H> void Submit(uint32_t slot, H2D&& h2d, Kernels&& kernels, D2H&& d2h) {
    Slot& s = slots_[slot];
    Record(s.t_in[0], s_in_);
    s.h2d_bytes = h2d((hipStream_t)s_in_);
    Record(s.t_in[1], s_in_);
    Record(s.h2d_done, s_in_);

    who_.Hip(hipStreamWaitEvent(s_compute_, s.h2d_done, 0), "hipStreamWaitEvent");
    Record(s.t_k[0], s_compute_);
    kernels((hipStream_t)s_compute_);
    Record(s.t_k[1], s_compute_);
    Record(s.compute_done, s_compute_);

    who_.Hip(hipStreamWaitEvent(s_out_, s.compute_done, 0), "hipStreamWaitEvent");
    Record(s.t_out[0], s_out_);
    s.d2h_bytes = d2h((hipStream_t)s_out_);
    Record(s.t_out[1], s_out_);
    Record(s.d2h_done, s_out_);

    s.busy = true;
    ++next_;
    if (next_ - delivered_ >= slots_.size() - 1) DeliverOldest();
  }

  // everything pending, in order; every slot is free afterwards
  const Totals& Finish() {
    while (delivered_ < next_) DeliverOldest();
    for (Slot& s : slots_) s.busy = false;  // everything delivered and synchronised
    totals_.wall_ms = MsSince(t_begin_);
    return totals_;
  }

 private:
  using Clock = std::chrono::steady_clock;
  static double MsSince(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

  struct Slot {
    Event h2d_done, compute_done, d2h_done;
    Event t_in[2], t_k[2], t_out[2];  // start / end of the batch's work on each stream
    uint64_t h2d_bytes = 0, d2h_bytes = 0;
    bool busy = false;
    explicit Slot(const Who& who) : h2d_done(who), compute_done(who), d2h_done(who) {
      for (Event* e : {&t_in[0], &t_in[1], &t_k[0], &t_k[1], &t_out[0], &t_out[1]}) *e = Event(who, true);
    }
  };

  void Record(hipEvent_t e, hipStream_t s) { who_.Hip(hipEventRecord(e, s), "hipEventRecord"); }
  double Elapsed(hipEvent_t a, hipEvent_t b) {
    float ms = 0;
    who_.Hip(hipEventElapsedTime(&ms, a, b), "hipEventElapsedTime");
    return ms;
  }
  void DeliverOldest() {
    const uint32_t slot = delivered_ % (uint32_t)slots_.size();
    Slot& s = slots_[slot];
    const Clock::time_point t0 = Clock::now();
    who_.Hip(hipEventSynchronize(s.d2h_done), "hipEventSynchronize");
    totals_.deliver_wait_ms += MsSince(t0);
    totals_.h2d_ms += Elapsed(s.t_in[0], s.t_in[1]);
    totals_.kernels_ms += Elapsed(s.t_k[0], s.t_k[1]);
    totals_.d2h_ms += Elapsed(s.t_out[0], s.t_out[1]);
    totals_.h2d_bytes += s.h2d_bytes; totals_.d2h_bytes += s.d2h_bytes;
    ++totals_.batches;
    ++delivered_;  // (first: the caller's deliver may throw)
    deliver_(slot);
  }

  Who who_;
  std::vector<Slot> slots_;  // (declared before the streams: those synchronise and go first)
  Stream s_in_, s_compute_, s_out_;
  uint32_t next_ = 0, delivered_ = 0;  // batches submitted / delivered since Begin: those in between are pending, in their slots
  Deliver deliver_;
  Totals totals_;
  Clock::time_point t_begin_;
};

}  // namespace host
}  // namespace svc
