"""Stateful tracking over video streams (reference: cvarArMultRegistration's `markers` in/out argument,
/root/reference/src/opencvar.cpp:619, 635-668 -- ARTest keeps one vector<CvarMarker> per camera across frames).

A stream is sequential (frame t needs the markers of frame t-1), streams are independent: one batch = the frame of the
same time step of every stream, batch lane s = stream s, and lane s's `prev` is what lane s returned one step
earlier.  Across GPUs, streams (not frames) are sharded: rank r owns the streams `streams_of(r, world, n)`."""
import numpy as np


def streams_of(rank, world, n_streams):
    """Streams owned by `rank`: contiguous blocks, sizes differing by at most one."""
    base, extra = divmod(n_streams, world)
    first = rank * base + min(rank, extra)
    return list(range(first, first + base + (1 if rank < extra else 0)))


class StreamTracker:
    """Carries each stream's markers from one call to the next, like the reference's caller does."""

    def __init__(self, detector, n_streams):
        self.det = detector
        self.prev = [[] for _ in range(n_streams)]

    def reset(self, stream=None):
        for s in (range(len(self.prev)) if stream is None else [stream]):
            self.prev[s] = []

    def step(self, frames, grey_in_place=False):
        """frames: uint8 [n_streams, H, W, 3] in host memory, the next frame of every stream.
        Returns (markers [n_streams, MAX_MARKERS], counts [n_streams]); the state advances."""
        assert len(frames) == len(self.prev)
        markers, counts = self.det.detect_host(frames, grey_in_place=grey_in_place, prev=self.prev)
        self.prev = [[markers[s, k].copy() for k in range(min(int(counts[s]), markers.shape[1]))] for s in range(len(self.prev))]
        return markers, counts


class DeviceStreamTracker:
    """StreamTracker for frames that are already in device memory, with every stream's records and its previous frame kept on
    the device between steps.  Each time step runs Detector.flow_records from the previous frames to the new ones (the records
    move to where the markers are now), then enqueue_tracked with the flowed records as `prev`, then results_to_device: the 20-px
    rule of the tracking stage compares detections with predicted corners, so a marker that moves more than 20 px per frame
    keeps its identity.  predict=False skips the flow step: the tracking stage sees the records where they were, as StreamTracker
    does.  Device memory comes from torch; all work of a step runs on one torch stream of the tracker's own."""

    def __init__(self, detector, n_streams, width, height, predict=True, params=None, fmt=None):
        import torch
        from . import FORMAT_BPP, MARKER_DTYPE, input_format_code
        self.det, self.n, self.width, self.height, self.predict, self.params = detector, n_streams, width, height, predict, params
        self.fmt = detector.input_format if fmt is None else input_format_code(fmt)
        self.frame_bytes = FORMAT_BPP[self.fmt] * width * height
        dev = torch.device("cuda", torch.cuda.current_device())
        self._torch = torch
        self._stream = torch.cuda.Stream(dev)
        self.recs = torch.zeros(n_streams * detector.max_markers * MARKER_DTYPE.itemsize, dtype=torch.uint8, device=dev)
        self.counts = torch.zeros(n_streams, dtype=torch.int32, device=dev)
        self.prev_frames = torch.zeros(n_streams * self.frame_bytes, dtype=torch.uint8, device=dev)
        self.have_prev = False

    def reset(self):
        """every stream starts again with no records"""
        with self._torch.cuda.stream(self._stream):
            self.counts.zero_()
        self.have_prev = False

    def step(self, frames, grey_in_place=False):
        """frames: a contiguous uint8 device tensor holding the next frame of every stream ([n_streams, H, W, bpp], or [n_streams,
        H, W] grey).  Returns (markers [n_streams, max_markers], counts [n_streams]) in host memory; the state advances."""
        torch, det = self._torch, self.det
        assert frames.is_cuda and frames.dtype == torch.uint8 and frames.is_contiguous() and frames.numel() == self.n * self.frame_bytes
        self._stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(self._stream):
            s = self._stream.cuda_stream
            if self.predict and self.have_prev:
                det.flow_records(self.prev_frames.data_ptr(), frames.data_ptr(), self.width, self.height, self.n, self.recs.data_ptr(),
                                 self.counts.data_ptr(), self.recs.data_ptr(), fmt=self.fmt, params=self.params, stream=s)
            if self.predict:
                self.prev_frames.copy_(frames.reshape(-1))   # (before the batch: grey_in_place changes the frames)
                self.have_prev = True
            det.enqueue_tracked(frames.data_ptr(), self.width, self.height, self.n, self.recs.data_ptr(), self.counts.data_ptr(),
                                grey_in_place=grey_in_place, stream=s)
            det.results_to_device(self.recs.data_ptr(), self.counts.data_ptr(), stream=s)
        frames.record_stream(self._stream)
        return det.collect()
