"""A clip that lives in HOST memory, through the same hot path: frames cross PCIe in batches on a
copy stream while the previous batch is in the kernels and the one before is on its way back
(frame batching + H2D / compute / D2H overlap).

The reference encodes synchronously, one frame per call, from pageable memory
(libs/encoder.cpp:472-498); the C++ drop-in wrappers of include/svc/motion.hpp keep that contract
and pay a PCIe round trip per call.  This is the batched form a host application would use
instead: it writes unpadded BGR frames into pinned input buffers handed out by the encoder and
reads motion vectors, region ids and coefficient planes (or wire records) from pinned output
buffers -- no pageable staging copy on either side.  Results are identical to ClipEncoder's on
the resident clip (same kernels, same RANSAC draws, same segmentation seeds).

The bench's `value` never comes from here (inputs resident in HBM is the contract); DESIGN.md
quotes this path's PCIe-inclusive rate next to it."""
from __future__ import annotations

from typing import Dict, Iterator, List, Optional

import numpy as np
import torch

from .configs import CodecConfig
from . import native
from .pipeline import ClipEncoder, ransac_samples


class _Slot:
    def __init__(self, cfg: CodecConfig, batch: int, device, wire: bool, segmentation: bool, compact: bool = False,
                 budget: Optional[int] = None, ladder=None, entropy: bool = False):
        # with a budget the transform leaves RAW planes and the pack picks each frame's steps
        self.enc = ClipEncoder(cfg, batch + 1, device, segmentation=segmentation, wire=wire, quantise=budget is None)
        pw, ph = cfg.padded
        self.pin_in = torch.zeros((batch + 1, ph, pw, 3), dtype=torch.uint8).pin_memory()  # padding stays zero
        e = self.enc
        self.pin_mv = torch.empty(e.mv.shape, dtype=torch.float32).pin_memory()
        self.pin_types = torch.empty(e.types.shape, dtype=torch.int32).pin_memory()
        self.pin_gm = torch.empty(e.gm.shape, dtype=torch.float32).pin_memory()
        big = e.records if e.wire else e.coeffs
        self.pin_big = torch.empty(big.shape, dtype=big.dtype).pin_memory() if big is not None and not compact else None
        self.compact = compact
        if compact:  # the quantised planes leave as the compact stream (levels.py): packed on the device, drained by a kernel
            cap = native.levels_max_bytes(batch, pw, ph, cfg.dct_block, cfg.mv_block)
            self.packed = torch.empty(cap, dtype=torch.uint8, device=device)
            self.offsets = torch.empty(batch + 1, dtype=torch.int64, device=device)
            ws = (native.pack_levels_workspace_bytes(batch, pw, ph, cfg.dct_block) if budget is None else
                  native.pack_levels_budget_workspace_bytes(batch, pw, ph, cfg.dct_block, len(ladder)))
            self.pack_ws = torch.empty(max(ws, 16), dtype=torch.uint8, device=device)
            self.pin_offsets = torch.empty(batch + 1, dtype=torch.int64).pin_memory()
            if entropy:  # the packed frames are then coded losslessly on the device ("SVCE", entropy.py) and only those drain
                cap = native.entropy_max_bytes(batch, pw, ph, cfg.dct_block, cfg.mv_block)
                self.coded = torch.empty(cap, dtype=torch.uint8, device=device)
                self.coded_offsets = torch.empty(batch + 1, dtype=torch.int64, device=device)
                ews = native.entropy_workspace_bytes(batch, pw, ph, cfg.dct_block, cfg.mv_block)
                self.entropy_ws = torch.empty(max(ews, 16), dtype=torch.uint8, device=device)
                self.entropy_status = torch.empty(batch, dtype=torch.int32, device=device)
                self.pin_entropy_status = torch.empty(batch, dtype=torch.int32).pin_memory()
            self.pin_packed = torch.empty(cap, dtype=torch.uint8).pin_memory()
        self.entropy = entropy
        self.budget = native.budget_tensor(budget, batch, device) if budget is not None else None
        self.ladder = ladder
        if budget is not None:
            self.choice = torch.empty(batch, dtype=torch.int32, device=device)
            self.pin_choice = torch.empty(batch, dtype=torch.int32).pin_memory()
        self.h2d_done = torch.cuda.Event()
        self.compute_done = torch.cuda.Event()
        self.d2h_done = torch.cuda.Event()
        self.busy = False
        self.count = 0      # encoded frames in flight in this slot
        self.first = 0      # index of its first encoded frame in the clip


class HostStreamEncoder:
    """encode(frames) yields, batch by batch, dicts of numpy views into pinned memory:
    first (index of the batch's first encoded frame; frame 0 of a clip is tracked-only,
    libs/encoder.cpp:361-367), mv (n, blocks, 2) f32, types (n, blocks) i32, gm (n, 2) f32 and
    coeffs (n, 3, H, W) f32 (quantised) or records (n, bytes) u8 -- the serialised RAW coefficients over the
    PADDED tile grid, what the reference's decoder parses (libs/decoder.cpp:185-186); the first batch of a wire
    stream also carries "header", the 32 bytes of libs/codec.hpp:8-17.  compact=True replaces coeffs by "compact",
    the used bytes of the compact quantised-coefficient stream (u8; levels.iter_frames reads it), and
    "compact_offsets" (n + 1,) i64.  compact_budget (bytes per frame, with compact and compact_ladder, a sequence of (fg_step,
    bg_step) pairs finest first, e.g. levels.step_ladder) packs each frame with the finest pair whose frame fits the budget
    (svc_hip_pack_levels_budget_frames) and adds "compact_choice" (n,) u32: the pair's index, bit 31 set where none fits.
    entropy=True (with compact, without a budget) codes every packed frame losslessly on the device, and "compact" /
    "compact_offsets" carry the "SVCE" frames (entropy.iter_frames decodes them to the SVCQ frames compact=True yields).
    A view is valid until depth - 2 more
    batches have been yielded (its slot is re-staged one iteration before its turn to be yielded comes again)."""

    def __init__(self, cfg: CodecConfig, batch: int = 32, device=None, wire: bool = False,
                 segmentation: bool = True, depth: int = 3, compact: bool = False, compact_budget: Optional[int] = None,
                 compact_ladder=None, entropy: bool = False):
        if compact and (wire or not cfg.dct_block):
            raise ValueError("compact output is a form of the quantised planes: not with wire records, nor without a transform")
        if compact_budget is not None and (not compact or compact_ladder is None or len(compact_ladder) == 0):
            raise ValueError("a byte budget needs compact output and a ladder of steps")
        if entropy and (not compact or compact_budget is not None):
            raise ValueError("entropy coding codes the compact stream (compact=True), and a budget counts uncoded bytes: "
                             "not with compact_budget")
        ladder = None if compact_budget is None else [(int(fg), int(bg)) for fg, bg in compact_ladder]
        self.cfg, self.batch, self.depth = cfg, batch, max(3, depth)  # 2 would leave nothing overlapped
        self.dev = device or torch.device("cuda")
        self.slots = [_Slot(cfg, batch, self.dev, wire, segmentation, compact, compact_budget, ladder, entropy)
                      for _ in range(self.depth)]
        self.copy_in = torch.cuda.Stream(device=self.dev)
        self.copy_out = torch.cuda.Stream(device=self.dev)
        self.compute = torch.cuda.Stream(device=self.dev)
        e = self.slots[0].enc
        self._iters, self._subset, self._blocks = e.iters, e.ransac["subset_sz"], e.blocks
        self._seg_seed0 = e.seg_seed

    def _stage(self, slot: _Slot, frames: np.ndarray, lo: int, hi: int, carry: bool) -> int:
        """Frames [lo, hi) of the clip into the slot's pinned input; returns the encoded-frame count."""
        h, w = frames.shape[1:3]
        n = hi - lo
        dst = slot.pin_in.numpy()
        off = 1 if carry else 0  # entry 0 = the previous batch's last frame, copied on the device
        dst[off:off + n, :h, :w] = frames[lo:hi]
        return n if carry else n - 1

    def encode(self, frames: np.ndarray) -> Iterator[Dict[str, np.ndarray]]:
        """frames: (N, h, w, 3) u8, unpadded, anywhere in host memory."""
        n_total = frames.shape[0]
        assert frames.dtype == np.uint8 and frames.shape[3] == 3 and n_total >= 2
        assert frames.shape[1] <= self.cfg.padded[1] and frames.shape[2] <= self.cfg.padded[0]
        samples = ransac_samples(n_total - 1, self._iters, self._subset, self._blocks, self.cfg.seed, self.dev)
        # the draws (and the slots' zero-initialised buffers) were produced on the caller's current stream:
        # the worker streams start behind it
        cur = torch.cuda.current_stream(self.dev)
        for s in (self.copy_in, self.compute, self.copy_out):
            s.wait_stream(cur)
        self._n_total = n_total
        B = self.batch
        pending: List[_Slot] = []
        prev: Optional[_Slot] = None
        lo, k, first = 0, 0, 1
        while lo < n_total:
            slot = self.slots[k % self.depth]
            if slot.busy:  # its results were handed out `depth` batches ago: the caller is done with the views
                slot.d2h_done.synchronize()
                slot.busy = False
            carry = prev is not None
            hi = min(n_total, lo + (B if carry else B + 1))
            cnt = self._stage(slot, frames, lo, hi, carry)
            e = slot.enc
            with torch.cuda.stream(self.copy_in):
                off = 1 if carry else 0
                e.bgr[off:off + (hi - lo)].copy_(slot.pin_in[off:off + (hi - lo)], non_blocking=True)
                if carry:
                    self.copy_in.wait_event(prev.h2d_done)
                    e.bgr[0].copy_(prev.enc.bgr[prev.count], non_blocking=True)  # its last frame, either way it was laid out
                slot.h2d_done.record(self.copy_in)
            g0 = first - 1  # global pair index of this batch's first pair
            e.seg_seed = self._seg_seed0 + g0
            with torch.cuda.stream(self.compute):
                # sliced on the stream that consumes them (torch.cat is a kernel)
                e.samples = samples[g0:g0 + e.pairs_per_step] if g0 + e.pairs_per_step <= n_total - 1 else \
                    torch.cat([samples[g0:], samples[:e.pairs_per_step - (n_total - 1 - g0)]])
                self.compute.wait_event(slot.h2d_done)
                e.step()
                if slot.budget is not None:
                    c_ = self.cfg
                    native.pack_levels_budget_frames(e.coeffs[:cnt], e.types[:cnt], c_.dct_block, c_.mv_block, slot.ladder,
                                                     slot.budget[:cnt], out=slot.packed, offsets=slot.offsets[:cnt + 1],
                                                     workspace=slot.pack_ws, choice=slot.choice[:cnt])
                elif slot.compact:
                    c_ = self.cfg
                    native.pack_levels_frames(e.coeffs[:cnt], e.types[:cnt], c_.dct_block, c_.mv_block, c_.fg_step, c_.bg_step,
                                              out=slot.packed, offsets=slot.offsets[:cnt + 1], workspace=slot.pack_ws)
                    if slot.entropy:
                        pw, ph = c_.padded
                        native.entropy_encode_frames(slot.packed, slot.offsets[:cnt + 1], pw, ph, c_.dct_block, c_.mv_block,
                                                     out=slot.coded, out_offsets=slot.coded_offsets[:cnt + 1],
                                                     workspace=slot.entropy_ws, status=slot.entropy_status[:cnt])
                slot.compute_done.record(self.compute)
            with torch.cuda.stream(self.copy_out):
                self.copy_out.wait_event(slot.compute_done)
                slot.pin_mv[:cnt].copy_(e.mv[:cnt], non_blocking=True)
                slot.pin_types[:cnt].copy_(e.types[:cnt], non_blocking=True)
                slot.pin_gm[:cnt].copy_(e.gm[:cnt], non_blocking=True)
                if slot.pin_big is not None:
                    big = e.records if e.wire else e.coeffs
                    slot.pin_big[:cnt].copy_(big[:cnt], non_blocking=True)
                if slot.compact:
                    c_ = self.cfg
                    pw, ph = c_.padded
                    if slot.entropy:
                        native.entropy_drain(slot.coded, slot.coded_offsets[:cnt + 1], pw, ph, c_.dct_block, c_.mv_block,
                                             slot.pin_packed)
                        slot.pin_offsets[:cnt + 1].copy_(slot.coded_offsets[:cnt + 1], non_blocking=True)
                        slot.pin_entropy_status[:cnt].copy_(slot.entropy_status[:cnt], non_blocking=True)
                    else:
                        native.levels_drain(slot.packed, slot.offsets[:cnt + 1], pw, ph, c_.dct_block, c_.mv_block, slot.pin_packed)
                        slot.pin_offsets[:cnt + 1].copy_(slot.offsets[:cnt + 1], non_blocking=True)
                if slot.budget is not None:
                    slot.pin_choice[:cnt].copy_(slot.choice[:cnt], non_blocking=True)
                slot.d2h_done.record(self.copy_out)
            slot.busy, slot.count, slot.first = True, cnt, first
            pending.append(slot)
            prev, lo, k, first = slot, hi, k + 1, first + cnt
            if len(pending) >= self.depth - 1:
                yield self._finish(pending.pop(0))
        while pending:
            yield self._finish(pending.pop(0))

    def _finish(self, slot: _Slot) -> Dict[str, np.ndarray]:
        slot.d2h_done.synchronize()
        c = slot.count
        out = {"first": slot.first, "mv": slot.pin_mv.numpy()[:c], "types": slot.pin_types.numpy()[:c],
               "gm": slot.pin_gm.numpy()[:c]}
        if slot.pin_big is not None:
            out["records" if slot.enc.wire else "coeffs"] = slot.pin_big.numpy()[:c]
        if slot.entropy:  # the coder's input is the pack's own output: a flagged frame is a bug, not a frame to pass on
            bad = np.flatnonzero(slot.pin_entropy_status.numpy()[:c])
            if bad.size:
                raise RuntimeError(f"svc_hip_entropy_encode_frames flagged frame {slot.first + int(bad[0])} with status "
                                   f"{int(slot.pin_entropy_status.numpy()[bad[0]])}")
        if slot.compact:
            offs = slot.pin_offsets.numpy()[:c + 1]
            out["compact"], out["compact_offsets"] = slot.pin_packed.numpy()[:int(offs[-1])], offs
        if slot.budget is not None:
            out["compact_choice"] = slot.pin_choice.numpy()[:c].view(np.uint32)
        if slot.enc.wire and slot.first == 1:
            c_ = self.cfg
            out["header"] = native.wire_header(self._n_total, c_.width, c_.height, c_.mv_block, c_.levels, c_.dct_block)
        return out
