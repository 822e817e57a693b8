"""Frames in, results out: the GPU side of the reference's inference loop as one double-buffered pipeline.

The reference's ``predict.py`` runs three processes (predict.py:45-122,250-255): a DataLoader that decodes and
preprocesses frames on the host (utils/dataset.py:145-161,310-330), ``Workers.predict`` (frames ``.to(device)``,
``net.predict``) and ``Workers.transfer_gpu_to_cpu`` (``preds_to_masks`` + ``.cpu().numpy()`` of every requested
output).  ``FramePipeline`` is the device part of that loop in ONE process with HIP streams instead of processes:

    host uint8 HWC frames (pinned) --copy stream--> GPU uint8 --HIP--> /255, HWC->CHW (+ INTER_AREA downscale)
        --> Reconstructor.predict_async (UNet on the caller's stream, ResNet-STN / warp / CE on its side stream)
        --> uint8 arg-max mask, uint8 warp mask, theta, consistency score, POI --copy stream--> pinned host arrays

Two slots alternate: while batch k computes, batch k + 1 uploads and batch k - 1 downloads.  Everything a batch needs
on the host arrives in its slot's pinned buffers; ``get()`` waits for that batch's download event only.

Every batch has its own TICKET (slot, generation, its own upload / download events).  The order a caller must keep is
checked, not assumed: ``submit`` refuses a slot whose previous batch was not collected; ``collect`` refuses to download
into host buffers whose previous batch was never fetched with ``get``; ``get`` refuses a ticket whose host buffers have
meanwhile been given to a later batch.  ``wait_uploaded(ticket)`` (or ``ticket.uploaded``) tells when the caller's host
frame buffer has been read and may be refilled.

Outputs and dtypes are those of predict.py:92-118 (``outputs.transfer_gpu_to_cpu`` is the synchronous version):
``segm_mask`` uint8 (B,H,W), ``warp_mask`` uint8 (B,H,W), ``theta`` float32 (B,1,3,3), ``consist_score`` float32 (B,),
``poi`` float32 (B,N,2).  With ``overlay=`` an ``OverlayRenderer`` and ``"overlay"`` requested, ``overlay`` uint8 (B,H,W,3): the
uploaded frames at their decoded size with the court drawn over them (sfh_amd.visualize; viz_preds.py's frames, without
the label - its text is the score, which is not on the host when the launch is enqueued).  With ``top_view=`` a
``mapping.TopViewRenderer``, ``top_view`` uint8 (B,hc,wc,3) and ``top_view_valid`` uint8 (B,hc,wc): the uploaded frames
rectified onto the court plane with the batch's own theta (sfh_amd.mapping).

With ``png=(names)`` the named image outputs (``segm_mask``, ``warp_mask``, ``overlay``, ``top_view``) are encoded on the device
(sfh_amd.pngenc) and arrive as ``"<name>_png"``, a list of B 1-D uint8 arrays holding PNG files; the raw image is then not
downloaded.  The files of a batch lie back to back behind their offsets and sizes in one device buffer, whose first
``png_budget`` bytes of file data travel with the offsets in ONE non-blocking copy; ``get()`` reads ``offsets[B]`` and fetches what
lies beyond the budget with one further, synchronous copy (label maps compress 18-70x: the default budget, an eighth of the
raw size of the output, is not exceeded by them).

With ``jpeg=(names)`` the photographic outputs (``overlay``, ``top_view``) are encoded on the device as baseline JPEG files of
quality ``jpeg_quality`` (sfh_amd.jpegenc) and arrive as ``"<name>_jpeg"`` in the same way, through the same single copy with a
budget (``jpeg_budget``, default a quarter of the raw size) and the same overflow fetch.  Masks hold class ids and stay PNG.
"""
import numpy as np
import torch

from . import engine as E
from . import outputs as O
from . import jpegenc as J
from . import jpegdec as JD
from . import pngenc as P
from . import resample as RS

PNG_OUTPUTS = ("segm_mask", "warp_mask", "overlay", "top_view")
JPEG_OUTPUTS = ("overlay", "top_view")


def png_head_bytes(batch):
    """bytes of offsets int64 (B+1) and sizes int32 (B) in front of the file data, padded to 16"""
    return (8 * (batch + 1) + 4 * batch + 15) // 16 * 16


def png_files_from_head(head, batch, budget, fetch_rest):
    """head: the downloaded first png_head_bytes(batch) + budget bytes of a PNG or JPEG buffer (1-D uint8 array) -> list of `batch` 1-D
    uint8 arrays.  fetch_rest(begin, end): the file data bytes [begin, end) as a 1-D uint8 array, called once and only when
    offsets[batch] exceeds the budget."""
    offsets = head[:8 * (batch + 1)].view(np.int64)
    sizes = head[8 * (batch + 1):8 * (batch + 1) + 4 * batch].view(np.int32)
    total = int(offsets[batch])
    data = head[png_head_bytes(batch):]
    if total > budget:
        rest = np.asarray(fetch_rest(budget, total), dtype=np.uint8)
        if rest.shape != (total - budget,):
            raise RuntimeError(f"FramePipeline: overflow fetch returned {rest.shape}, expected ({total - budget},)")
        data = np.concatenate([data[:budget], rest])
    return P.split_files(data, offsets, sizes)


# ONE copy stream per device, shared by every FramePipeline of the process, for uploads AND downloads.  HIP multiplexes streams
# onto a handful of hardware queues (four by default) in creation order: with an upload stream and a download stream per pipeline
# object, every second pipeline a process created got streams that share a queue with the model's compute / side streams, and its
# copies then waited behind kernels (measured: 13.2 ms per batch from the first pipeline, 14.2 from the second, 13.3 from the third
# ...; 13.7 / 16.0 with 1920x1080 frames; GPU_MAX_HW_QUEUES=8 removes the alternation: profiles/micro/e2e_parity_probe.py).  The
# two directions need no stream of their own: an upload is 0.25-1.9 ms, a download 0.14 ms, per 13 ms batch.
_COPY_STREAMS = {}


def _copy_stream(dev):
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    st = _COPY_STREAMS.get(key)
    if st is None:
        st = _COPY_STREAMS[key] = torch.cuda.Stream(dev)
    return st


def _copied(res):
    """a result dict that outlives the slot's pinned buffers (the PNG lists are copies already)"""
    return {k: (v if isinstance(v, list) else np.array(v)) for k, v in res.items()}


class Ticket:
    """one submitted batch: which slot it uses, its generation on that slot, its own events"""
    __slots__ = ("slot", "gen", "uploaded", "downloaded", "handle", "dev", "fetched")

    def __init__(self, slot, gen):
        self.slot, self.gen = slot, gen
        self.uploaded = self.downloaded = self.handle = self.dev = None
        self.fetched = False


class FramePipeline:
    def __init__(self, net, batch, frame_hw, req_outputs=("theta", "warp_mask"), consistency=False, channels=3, overlay=None,
                 top_view=None, png=None, png_budget=None, jpeg=None, jpeg_quality=90, jpeg_budget=None, resize="area",
                 jpeg_in_max_bytes=None):
        """net: a Reconstructor on the GPU in eval mode; frame_hw = (H, W) of the DECODED frames (net.unet_size, or any
        larger size: cv2.INTER_AREA's downscale runs on the GPU, engine.frames_u8_to_input); req_outputs as predict.py's --req_outputs.
        overlay: a visualize.OverlayRenderer for the output "overlay" (its score is the consistency score: without
        consistency the renderer must be source="warp" or "segm" and have no overlay threshold).
        top_view: a mapping.TopViewRenderer for the outputs "top_view" and "top_view_valid" (its score is the consistency score:
        a renderer with max_score needs consistency=True).
        png: names among PNG_OUTPUTS to deliver as PNG files encoded on the device ("<name>_png") instead of raw images;
        png_budget: bytes of file data per output and batch downloaded with the offsets (default: raw size / 8).
        jpeg: names among JPEG_OUTPUTS to deliver as JPEG files of quality jpeg_quality encoded on the device ("<name>_jpeg")
        instead of raw images; jpeg_budget as png_budget (default: raw size / 4).  A name may be in png or in jpeg, not both.
        resize: how frames of another size than net.unet_size get there.  "area" (the default): cv2.INTER_AREA, VideoDataset's
        rule, downscales only; overlay and top_view are drawn from the frames at their decoded size.  "pil": Pillow's
        Image.resize (bicubic), BasicDataset's rule (sfh_amd.resample), any size pair within its tap bound; overlay and top_view
        are drawn from the RESIZED frames, as they are when the same frames come resized from the host.
        jpeg_in_max_bytes: the longest file ``submit_jpeg`` admits (default: jpegenc.jpeg_capacity of the frame size); it sizes
        the decoders' buffers, which are allocated at the first ``submit_jpeg``."""
        self.jpeg_in_max_bytes = jpeg_in_max_bytes
        if resize not in ("area", "pil"):
            raise ValueError(f'FramePipeline: resize={resize!r} ("area" or "pil")')
        self.net, self.B = net, int(batch)
        self.req = set(req_outputs)
        self.consistency = bool(consistency) or "consistency" in self.req
        self.poi = "poi" in self.req
        self.overlay = None
        if "overlay" in self.req:
            if overlay is None:
                raise ValueError('FramePipeline: the output "overlay" needs overlay=OverlayRenderer(...)')
            if not self.consistency and (overlay.source == "auto" or overlay.overlay_threshold is not None):
                raise ValueError('FramePipeline: without consistency=True there is no score - the OverlayRenderer must be '
                                 'source="warp" or "segm" and have no overlay_threshold')
            if channels != 3:
                raise ValueError(f'FramePipeline: the output "overlay" needs 3-channel frames, not {channels}')
            self.overlay = overlay
        self.top_view = None
        if top_view is not None:
            if channels != 3:
                raise ValueError(f'FramePipeline: the output "top_view" needs 3-channel frames, not {channels}')
            if top_view.max_score is not None and not self.consistency:
                raise ValueError('FramePipeline: without consistency=True there is no score - the TopViewRenderer must have '
                                 'no max_score')
            self.top_view = top_view
        p = next(net.parameters())
        if p.device.type != "cuda":
            raise RuntimeError("FramePipeline needs the model on the GPU (no CPU fallback)")
        self.dev = dev = p.device
        H, W = int(frame_hw[0]), int(frame_hw[1])
        tw, th = net.unet_size
        self.target = None if (W, H) == (tw, th) else (tw, th)
        self.resampler = None
        if resize == "pil" and self.target is not None:
            self.resampler = RS.resampler((H, W), (th, tw), channels)
            vh, vw = th, tw                               # the size of the frames overlay and top_view see
        else:
            vh, vw = H, W
        wh, ww = net._warp_hw
        nc = net.mask_classes
        self.h2d = self.d2h = _copy_stream(dev)
        pin = lambda shape, dt: torch.empty(shape, dtype=dt).pin_memory()
        self.png = tuple(png) if png else ()
        for name in self.png:
            if name not in PNG_OUTPUTS:
                raise ValueError(f"FramePipeline: png output {name!r} (one of {PNG_OUTPUTS})")
        # name -> (H, W, C) of every image output that can be encoded
        shapes = {}
        if "segm_mask" in self.req:
            shapes["segm_mask"] = (net.target_size[1], net.target_size[0], 1)
        if "warp_mask" in self.req and net.warper:
            shapes["warp_mask"] = (wh, ww, 1)
        if self.overlay is not None:
            shapes["overlay"] = (vh, vw, 3)
        if self.top_view is not None:
            shapes["top_view"] = (self.top_view.out_size[1], self.top_view.out_size[0], 3)
        self.jpeg = tuple(jpeg) if jpeg else ()
        for name in self.jpeg:
            if name not in JPEG_OUTPUTS:
                raise ValueError(f"FramePipeline: jpeg output {name!r} (one of {JPEG_OUTPUTS})")
            if name in self.png:
                raise ValueError(f"FramePipeline: output {name!r} is named in both png= and jpeg=")
        # name -> (encoder, budget, key suffix) of every output that leaves as files
        self._coded = {}
        for name in self.png + self.jpeg:
            fmt = "png" if name in self.png else "jpeg"
            if name not in shapes:
                raise ValueError(f"FramePipeline: {fmt} output {name!r} is not among this pipeline's outputs {sorted(shapes)}")
            h, w, c = shapes[name]
            given = png_budget if fmt == "png" else jpeg_budget
            budget = self.B * h * w * c // (8 if fmt == "png" else 4) if given is None else int(given)
            if budget < 0:
                raise ValueError(f"FramePipeline: {fmt}_budget {given}")
            if fmt == "png":
                enc = P.PngEncoder(h, w, c, self.B, bgr=True, device=dev)
            else:
                enc = J.JpegEncoder(h, w, c, self.B, quality=jpeg_quality, bgr=True, device=dev)
            self._coded[name] = (enc, min(budget, self.B * enc.capacity), "_" + fmt)
        self.slots = []
        for _ in range(2):
            # pending: the ticket submitted on this slot and not yet collected; collected: the ticket whose results the host
            # buffers hold (or are receiving)
            s = {"u8": torch.empty((self.B, H, W, channels), dtype=torch.uint8, device=dev),
                 "consumed": None, "host": {}, "pending": None, "collected": None, "gen": 0}
            if self.overlay is not None:
                s["overlay"] = torch.empty((self.B, vh, vw, 3), dtype=torch.uint8, device=dev)
                if "overlay" not in self._coded:
                    s["host"]["overlay"] = pin((self.B, vh, vw, 3), torch.uint8)
            if self.top_view is not None:
                wc, hc = self.top_view.out_size
                s["top_view"] = {"top_view": torch.empty((self.B, hc, wc, 3), dtype=torch.uint8, device=dev),
                                 "valid": torch.empty((self.B, hc, wc), dtype=torch.uint8, device=dev)}
                if "top_view" not in self._coded:
                    s["host"]["top_view"] = pin((self.B, hc, wc, 3), torch.uint8)
                s["host"]["top_view_valid"] = pin((self.B, hc, wc), torch.uint8)
            if "segm_mask" in self.req and "segm_mask" not in self._coded:
                s["host"]["segm_mask"] = pin((self.B, net.target_size[1], net.target_size[0]), torch.uint8)
            if "warp_mask" in self.req and net.warper and "warp_mask" not in self._coded:
                s["host"]["warp_mask"] = pin((self.B, wh, ww), torch.uint8)
            if "theta" in self.req:
                s["host"]["theta"] = pin((self.B, 1, 3, 3), torch.float32)
            if self.consistency and net.warper and net.use_unet:
                s["host"]["consist_score"] = pin((self.B,), torch.float32)
            if self.poi:
                s["host"]["poi"] = pin((self.B,) + tuple(net.court_poi.shape[1:]), torch.float32)
            # per encoded output: one device buffer [offsets | sizes | file data] and the pinned image of its first bytes
            s["png"] = {}
            for name, (enc, budget, _) in self._coded.items():
                hb = png_head_bytes(self.B)
                blob = torch.empty(hb + self.B * enc.capacity, dtype=torch.uint8, device=dev)
                batch_out = P.PngBatch(blob[hb:], blob[:8 * (self.B + 1)].view(torch.int64),
                                       blob[8 * (self.B + 1):8 * (self.B + 1) + 4 * self.B].view(torch.int32))
                s["png"][name] = {"blob": blob, "out": batch_out, "head": pin((hb + budget,), torch.uint8)}
            self.slots.append(s)
        self.k = 0
        self._nc = nc

    def submit(self, frames_u8_host):
        """frames_u8_host: uint8 (B,H,W,C) host tensor (pinned for a truly asynchronous upload).  Enqueues upload,
        preprocessing and the forward pass of this batch and returns its Ticket; nothing here waits for the GPU.  The host
        buffer is read asynchronously: refill it only after wait_uploaded(ticket)."""
        s = self.slots[self.k % 2]
        if s["pending"] is not None:
            raise RuntimeError("FramePipeline: collect() the batch submitted two calls ago before reusing its slot")
        self.k += 1
        s["gen"] += 1
        t = Ticket(s, s["gen"])
        cur = torch.cuda.current_stream(self.dev)
        with torch.cuda.stream(self.h2d):
            if s["consumed"] is not None:
                self.h2d.wait_event(s["consumed"])       # the preprocessing kernel that read this buffer last is done
            s["u8"].copy_(frames_u8_host, non_blocking=True)
            t.uploaded = torch.cuda.Event()
            t.uploaded.record(self.h2d)
        cur.wait_event(t.uploaded)
        return self._forward(s, t, cur)

    def submit_jpeg(self, files):
        """files: B JPEG files of the pipeline's frame size as bytes / 1-D uint8 arrays (or a jpegenc.JpegBatch), in the place of
        ``submit``'s decoded frames: the files and their parse tables are uploaded in one copy, decoded on the compute stream
        into the slot's frame buffer (sfh_amd.jpegdec: PIL's pixels, in BGR order), and then runs exactly what ``submit``
        runs.  The headers are parsed here, on the host: a refused file raises before anything is enqueued.  The files are
        copied into the slot's pinned staging buffer before this returns, so they need not outlive the call."""
        s = self.slots[self.k % 2]
        if s["pending"] is not None:
            raise RuntimeError("FramePipeline: collect() the batch submitted two calls ago before reusing its slot")
        if "jpegdec" not in s:
            _, H, W, C = s["u8"].shape
            s["jpegdec"] = JD.JpegDecoder(H, W, C, self.B, bgr=True, max_file_bytes=self.jpeg_in_max_bytes, device=self.dev)
        dec = s["jpegdec"]
        n = len(files.sizes) if isinstance(files, J.JpegBatch) else len(files)
        if n != self.B:
            raise ValueError(f"FramePipeline.submit_jpeg: {n} files for a batch of {self.B}")
        dec.stage(files)                                  # host only; raises for a refused file
        self.k += 1
        s["gen"] += 1
        t = Ticket(s, s["gen"])
        cur = torch.cuda.current_stream(self.dev)
        with torch.cuda.stream(self.h2d):
            if getattr(dec, "decoded", None) is not None:
                self.h2d.wait_event(dec.decoded)          # the slot's previous decode has read the device copy of the files
            dec.upload()
            t.uploaded = torch.cuda.Event()
            t.uploaded.record(self.h2d)
        cur.wait_event(t.uploaded)
        dec.decode_staged(out=s["u8"])                    # on cur: ordered behind every launch that read s["u8"]
        dec.decoded = torch.cuda.Event()
        dec.decoded.record(cur)
        return self._forward(s, t, cur)

    def _forward(self, s, t, cur):
        if self.resampler is not None:
            s["frames"], x = self.resampler.both(s["u8"])     # one launch: the resized bytes for overlay / top_view and / 255
        else:
            s["frames"] = s["u8"]
            x = E.frames_u8_to_input(s["u8"], self.target)
        s["consumed"] = torch.cuda.Event()
        s["consumed"].record(cur)
        t.handle = self.net.predict_async(x, consistency=self.consistency, project_poi=self.poi)
        s["pending"] = t
        return t

    def wait_uploaded(self, ticket):
        """block until the host frame buffer given to submit() has been read: it may be refilled afterwards"""
        ticket.uploaded.synchronize()

    def collect(self, ticket):
        """Enqueue post-processing and the download of a submitted batch (call it after submitting the NEXT batch, so
        that this batch's ResNet-STN / warp ran under that one's UNet).  Returns at once; get() waits."""
        t, s = ticket, ticket.slot
        if s["pending"] is not t:
            raise RuntimeError("FramePipeline.collect: this ticket is not the batch pending on its slot (collected already, "
                               "or from another pipeline)")
        prev = s["collected"]
        if prev is not None and not prev.fetched:
            raise RuntimeError("FramePipeline.collect: the slot's host buffers still hold a batch that was never fetched with "
                               "get(); this download would overwrite it")
        out = t.handle.result()                          # orders the current stream behind the batch
        t.handle = None
        cur = torch.cuda.current_stream(self.dev)
        devout = {}
        if "segm_mask" in s["host"] or "segm_mask" in self._coded:
            devout["segm_mask"] = O.format_masks(out["logits"], "gray", self._nc)          # uint8 arg-max (postprocess.py:7-18)
        if "warp_mask" in s["host"] or "warp_mask" in self._coded:
            devout["warp_mask"] = O.format_masks(out["warp_mask"].contiguous(), "gray", self._nc)   # int32 -> uint8 on the GPU
        for k in ("theta", "consist_score", "poi"):
            if k in s["host"]:
                devout[k] = out[k]
        if self.overlay is not None:
            # drawn from the slot's uploaded frames: the next upload into them waits for this launch too
            devout["overlay"] = self.overlay(s["frames"], out["theta"], score=out.get("consist_score"), segm=out.get("logits"),
                                             poi=out.get("poi") if self.overlay.marker_radius > 0 else None, out=s["overlay"])
            s["consumed"] = torch.cuda.Event()
            s["consumed"].record(cur)
        if self.top_view is not None:
            # rectified from the slot's uploaded frames, like the overlay: the next upload into them waits for this launch
            tv = self.top_view(s["frames"], out["theta"], score=out.get("consist_score"), out=s["top_view"])
            devout["top_view"], devout["top_view_valid"] = tv["top_view"], tv["valid"]
            s["consumed"] = torch.cuda.Event()
            s["consumed"].record(cur)
        for name, (enc, _, _) in self._coded.items():   # two launches per output; the raw image stays on the device
            raw = devout.pop(name)
            enc.encode(raw, out=s["png"][name]["out"])
        ready = torch.cuda.Event()
        ready.record(cur)
        with torch.cuda.stream(self.d2h):
            self.d2h.wait_event(ready)
            for k, v in devout.items():
                s["host"][k].copy_(v, non_blocking=True)
                v.record_stream(self.d2h)
            for name, pb in s["png"].items():
                pb["head"].copy_(pb["blob"][:pb["head"].numel()], non_blocking=True)
            t.downloaded = torch.cuda.Event()
            t.downloaded.record(self.d2h)
        t.dev = devout
        s["pending"], s["collected"] = None, t
        return t

    def get(self, ticket):
        """-> {name: numpy array} of a collected batch (views of the slot's pinned buffers: valid until the NEXT batch of this
        slot is collected, copy what must live longer)."""
        t, s = ticket, ticket.slot
        if t.downloaded is None:
            raise RuntimeError("FramePipeline.get: collect() this batch first")
        if s["collected"] is not t:
            raise RuntimeError(f"FramePipeline.get: the slot's host buffers now hold generation {s['collected'].gen}, this ticket "
                               f"is generation {t.gen} - fetch a batch before the batch two submissions later is collected")
        t.downloaded.synchronize()
        t.dev = None
        t.fetched = True
        res = {k: v.numpy() for k, v in s["host"].items()}
        for name, pb in s["png"].items():
            _, budget, suffix = self._coded[name]
            # the slot's device buffer is rewritten only by the collect() of a later batch, which needs this get() first
            res[name + suffix] = png_files_from_head(pb["head"].numpy(), self.B, budget,
                                                     lambda a, e, pb=pb: pb["out"].data[a:e].cpu().numpy())
        return res

    def run(self, batches, jpeg=False):
        """Generator over host uint8 batches (jpeg=True: over lists of B JPEG files, through ``submit_jpeg``) -> result dicts
        (copies), two batches in flight.  The producer may hand over the
        SAME pinned buffer every time: the next item is pulled from `batches` only after the upload of the batch just
        submitted has read its buffer (wait_uploaded) - with the one copy stream per device that upload queues behind the
        download of the batch two submissions back, so without the wait a producer that refills one buffer would overwrite
        frames still waiting to be copied."""
        prev = None
        done = None
        it = iter(batches)
        fr = next(it, None)
        while fr is not None:
            t = self.submit_jpeg(fr) if jpeg else self.submit(fr)
            if done is not None:
                yield _copied(self.get(done))
                done = None
            if prev is not None:
                done = self.collect(prev)
            prev = t
            self.wait_uploaded(t)
            fr = next(it, None)
        if done is not None:
            yield _copied(self.get(done))
        if prev is not None:
            yield _copied(self.get(self.collect(prev)))
