"""Batched MI355X RX engine: thin Python over the C ABI (include/ria_gpu.h).

`RxEngine` owns one ria_gpu handle (one modulation/code-rate pair, like one configured IWaveform).
All heavy lifting happens in libria_gpu.so; torch only provides device buffers and streams.
There is no CPU fallback: constructing an engine without a HIP device raises.
"""
import ctypes as C

import numpy as np
import torch

from . import capi


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class ChasePool:
    """A pool of device-resident HARQ chase caches (ria_gpu_chase_create): one fec::ChaseCache per link or trial.  Owned by
    the engine's handle: close it before the engine, or let the engine's close free it."""
    ENTRY = np.dtype([("last_access_ms", "<u8"), ("order", "<u8"), ("src_hash", "<u4"), ("dst_hash", "<u4"), ("seq", "<u2"),
                      ("used", "u1"), ("total_cw", "u1"), ("frame_type", "u1"), ("reserved", "u1", 3), ("combine_count", "u1", 16),
                      ("decoded", "u1", 16), ("has_sum", "u1", 16)])
    STATS = ("cache_hits", "cache_misses", "stores", "combines", "entries_evicted", "entries_expired", "recoveries")

    def __init__(self, engine, n_caches, max_entries=16, ttl_ms=30000):
        self.engine, self.lib = engine, engine.lib
        self.n_caches, self.max_entries, self.ttl_ms = int(n_caches), int(max_entries), int(ttl_ms)
        cfg = capi.ChaseConfig()
        self.lib.ria_gpu_chase_default_config(C.byref(cfg))
        cfg.n_caches, cfg.max_entries, cfg.ttl_ms = self.n_caches, self.max_entries, self.ttl_ms
        p = C.c_void_p()
        engine._check(self.lib.ria_gpu_chase_create(engine.h, C.byref(cfg), C.byref(p)))
        self.p = p

    def close(self):
        if getattr(self, "p", None) and getattr(self.engine, "h", None):
            self.lib.ria_gpu_chase_destroy(self.p)
        self.p = None

    def clear(self, cache_ids=None):
        """ChaseCache::clear for the listed caches (None: all; an empty list: none); counters stay"""
        ids = None
        if cache_ids is not None:
            ids = torch.as_tensor(np.ascontiguousarray(cache_ids, np.int32)).to(self.engine.device)
            if ids.numel() == 0:           # an empty tensor has no address, and a NULL list would mean every cache
                return
        self.engine._check(self.lib.ria_gpu_chase_clear(self.p, _ptr(ids), 0 if ids is None else ids.numel(), _stream_ptr()))

    def stats(self, cache_id):
        st = capi.ChaseStats()
        self.engine._check(self.lib.ria_gpu_chase_stats(self.p, int(cache_id), C.byref(st)))
        return {k: int(getattr(st, k)) for k in self.STATS}

    def export(self, cache_id):
        """(entries structured array [size()], sums float32 [size(), 16, 648], zero where has_sum is 0)"""
        ent = np.zeros(self.max_entries, self.ENTRY)
        sums = np.zeros((self.max_entries, 16, 648), np.float32)
        n = self.lib.ria_gpu_chase_export(self.p, int(cache_id), ent.ctypes.data, sums.ctypes.data)
        if n < 0:
            self.engine._check(n)
        return ent[:n], sums[:n]


class RxEngine:
    def __init__(self, modulation="QAM16", code_rate="R1_2", device=0, max_batch=4096):
        if not torch.cuda.is_available():
            raise capi.RiaError("ria_amd needs a HIP device (MI355X); there is no CPU fallback")
        self.lib = capi.load()
        self.modulation = capi.MOD[modulation] if isinstance(modulation, str) else int(modulation)
        self.code_rate = capi.RATE[code_rate] if isinstance(code_rate, str) else int(code_rate)
        cfg = capi.Config()
        self.lib.ria_gpu_default_config(C.byref(cfg))
        cfg.device = device
        cfg.modulation = self.modulation
        cfg.code_rate = self.code_rate
        cfg.max_batch = max_batch
        h = C.c_void_p()
        rc = self.lib.ria_gpu_create(C.byref(cfg), C.byref(h))
        if rc != capi.RIA_OK:
            raise capi.RiaError(f"ria_gpu_create failed with status {rc}")
        self.h = h
        self.cfg = cfg
        self.device = torch.device("cuda", device)
        self.geo = capi.Geometry()
        self._check(self.lib.ria_gpu_get_geometry(self.h, C.byref(self.geo)))

    def close(self):
        if getattr(self, "h", None):
            self.lib.ria_gpu_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != capi.RIA_OK:
            raise capi.RiaError(f"libria_gpu status {rc}: {self.lib.ria_gpu_last_error(self.h).decode()}")

    def set_split_parts(self, parts):
        """How many parts ria_gpu_rx_batch cuts a large batch into (internal streams); 0 = library default."""
        self._check(self.lib.ria_gpu_set_option(self.h, capi.OPT_SPLIT_PARTS, int(parts)))

    def set_dual_decoder(self, mode):
        """1: two codewords per wave in the retry kernels, -1: one, 0: library default"""
        self._check(self.lib.ria_gpu_set_option(self.h, capi.OPT_DUAL_DECODER, int(mode)))

    def set_fallback_queue_all(self, on):
        """1: the recovery fill also runs the fallback re-decodes no trial can read (as before the relevance rule); 0: default"""
        self._check(self.lib.ria_gpu_set_option(self.h, capi.OPT_FALLBACK_QUEUE_ALL, int(on)))

    def recovery_counts(self, slot=0):
        """Counters of the last CRC recovery on stream slot `slot`: frames flagged, frames reaching the fallback stage,
        codewords with re-decodes queued, (codeword, factor) re-decodes queued.  Synchronises the device."""
        out = (C.c_uint32 * 4)()
        self._check(self.lib.ria_gpu_debug_recovery_counts(self.h, int(slot), out))
        return {"flagged": int(out[0]), "fallback": int(out[1]), "list2": int(out[2]), "queued": int(out[3])}

    def set_state_exit(self, on):
        """1 (default): the retry kernels end a failing decode whose message state repeats (R1/2, R1/3); 0: every failing decode
        runs to its end"""
        self._check(self.lib.ria_gpu_set_option(self.h, capi.OPT_STATE_EXIT, int(on)))

    def state_exits(self, slot=0):
        """Decodes the repeated-state exit ended in the last decode call on stream slot `slot` (parts 1.. of a split rx call use
        slots 1..): all, phase 0, cascade, recovery fill.  Synchronises the device."""
        out = (C.c_uint32 * 4)()
        self._check(self.lib.ria_gpu_debug_state_exits(self.h, int(slot), out))
        return {"all": int(out[0]), "phase0": int(out[1]), "cascade": int(out[2]), "fill": int(out[3])}

    def first_decodes(self, slot=0):
        """First decodes (factor 0.9375) of the last decode call on stream slot `slot`: skipped behind a failed codeword of the
        frame, and made late behind a phase-0 rescue.  Synchronises the device."""
        out = (C.c_uint32 * 2)()
        self._check(self.lib.ria_gpu_debug_first_decodes(self.h, int(slot), out))
        return {"skipped": int(out[0]), "late": int(out[1])}

    # ---- helpers
    def _meta(self, n, cfo_hz, abs_pos, flags):
        if cfo_hz is None and abs_pos is None and flags is None:
            return None
        m = np.zeros(n, dtype=np.dtype([("cfo_hz", "<f4"), ("flags", "<u4"), ("abs_position", "<u8")]))
        if cfo_hz is not None:
            m["cfo_hz"] = cfo_hz
        if abs_pos is not None:
            m["abs_position"] = abs_pos
        if flags is not None:
            m["flags"] = flags
        return torch.from_numpy(m.view(np.uint8).reshape(n, 16)).to(self.device)

    @staticmethod
    def _status_array(t, dtype):
        return t.cpu().numpy().view(dtype).reshape(-1)

    FRAME_STATUS = np.dtype([("snr_db", "<f4"), ("cfo_hz", "<f4"), ("fading_index", "<f4"),
                             ("noise_variance", "<f4"), ("lts_phase_slope", "<f4"), ("snr_linear", "<f4"),
                             ("corr_phase", "<f4"), ("n_llr", "<i4")])
    DECODE_STATUS = np.dtype([("cw_ok", "u1", 4), ("iterations", "<u2", 4), ("attempts", "u1", 4),
                              ("frame_valid", "u1"), ("needs_recovery", "u1"), ("reserved", "u1", 2)])

    # ---- batched calls (device tensors in, device tensors out)
    def _frames_in(self, samples, offsets):
        """(n_frames, offsets tensor or None): either [n, frame_samples] rows, or one capture + uint64 sample offsets"""
        assert samples.dtype == torch.float32 and samples.is_contiguous()
        if offsets is None:
            assert samples.dim() == 2 and samples.shape[1] == self.geo.frame_samples
            return samples.shape[0], None
        off = np.ascontiguousarray(offsets, np.uint64)
        assert off.size == 0 or int(off.max()) + self.geo.frame_samples <= samples.numel(), "frame runs past the capture"
        return len(off), torch.from_numpy(off.view(np.int64)).to(self.device)

    def demod(self, samples, cfo_hz=None, abs_pos=None, flags=None, want_status=True, offsets=None):
        """samples: float32 [n_frames, frame_samples] on the GPU (or one capture + per-frame sample offsets)
        -> (llr [n, llrs_per_frame], status)"""
        n, off = self._frames_in(samples, offsets)
        llr = torch.empty((n, self.geo.llrs_per_frame), dtype=torch.float32, device=self.device)
        st = torch.zeros((n, 32), dtype=torch.uint8, device=self.device) if want_status else None
        meta = self._meta(n, cfo_hz, abs_pos, flags)
        self._check(self.lib.ria_gpu_demod_batch(self.h, _ptr(samples), _ptr(off), _ptr(meta), n, _ptr(llr), _ptr(st),
                                                 _stream_ptr()))
        return llr, st

    def decode(self, llr, flags=capi.DECODE_FULL):
        """llr: float32 [n_frames, >=2592] -> (info bytes [n, info_bytes_per_frame], status)"""
        n = llr.shape[0]
        assert llr.dtype == torch.float32 and llr.is_contiguous() and llr.shape[1] >= 2592
        info = torch.empty((n, self.geo.info_bytes_per_frame), dtype=torch.uint8, device=self.device)
        st = torch.zeros((n, 20), dtype=torch.uint8, device=self.device)
        self._check(self.lib.ria_gpu_decode_batch(self.h, _ptr(llr), llr.shape[1], n, flags, _ptr(info), _ptr(st),
                                                  _stream_ptr()))
        return info, st

    DFRAME_RESULT = np.dtype([("success", "u1"), ("codewords_ok", "u1"), ("codewords_failed", "u1"), ("frame_type", "u1"),
                              ("path", "u1"), ("header_total_cw", "u1"), ("stages", "u1"), ("reserved0", "u1"),
                              ("frame_bytes", "<i4"), ("iters_r14", "<u2"), ("iters_cw0", "<u2"), ("tries_r14", "u1"),
                              ("tries_rate", "u1"), ("reserved1", "u1", 2), ("reserved", "<i4", 3)])

    def decode_frame(self, llr, n_llr=None, flags=capi.DECODE_FULL, want_info=False):
        """StreamingDecoder::decodeFrame (OFDM branch) over rows of soft bits: llr float32 [n, 648 .. 32 * 648], n_llr the
        soft bits of each row (None: the whole row).  Returns (frame bytes uint8 [n, max(4, cols // 648) * bytes_per_codeword],
        result structured array (DFRAME_RESULT), decode status of the fixed attempt[, its codeword bytes])."""
        n, stride = llr.shape
        assert llr.dtype == torch.float32 and llr.is_contiguous()
        row = max(4, stride // 648) * self.geo.bytes_per_codeword
        frames = torch.empty((n, row), dtype=torch.uint8, device=self.device)
        res = torch.empty((n, 32), dtype=torch.uint8, device=self.device)
        st = torch.empty((n, 20), dtype=torch.uint8, device=self.device)
        info = torch.empty((n, self.geo.info_bytes_per_frame), dtype=torch.uint8, device=self.device) if want_info else None
        nl = None
        if n_llr is not None:
            nl = torch.as_tensor(np.ascontiguousarray(n_llr, np.int32)).to(self.device) if not torch.is_tensor(n_llr) else n_llr
            assert nl.dtype == torch.int32 and nl.numel() == n and nl.is_contiguous()
        self._check(self.lib.ria_gpu_decode_frame_batch(self.h, _ptr(llr), stride, _ptr(nl), n, flags, _ptr(frames), row,
                                                        _ptr(res), _ptr(st), _ptr(info), _stream_ptr()))
        out = (frames, self._status_array(res, self.DFRAME_RESULT), st)
        return out + (info,) if want_info else out

    def rx(self, samples, flags=capi.DECODE_FULL, cfo_hz=None, abs_pos=None, meta_flags=None, want_llr=False,
           out=None, offsets=None):
        """Fused samples -> payload bytes. Returns (info, decode_status[, llr, frame_status])."""
        n, off = self._frames_in(samples, offsets)
        if out is None:
            info = torch.empty((n, self.geo.info_bytes_per_frame), dtype=torch.uint8, device=self.device)
            st = torch.zeros((n, 20), dtype=torch.uint8, device=self.device)
        else:
            info, st = out
        llr = fst = None
        if want_llr:
            llr = torch.empty((n, self.geo.llrs_per_frame), dtype=torch.float32, device=self.device)
            fst = torch.zeros((n, 32), dtype=torch.uint8, device=self.device)
        meta = self._meta(n, cfo_hz, abs_pos, meta_flags)
        self._check(self.lib.ria_gpu_rx_batch(self.h, _ptr(samples), _ptr(off), _ptr(meta), n, flags, _ptr(info), _ptr(st),
                                              _ptr(llr), _ptr(fst), _stream_ptr()))
        return (info, st, llr, fst) if want_llr else (info, st)

    def ldpc_decode(self, llr_rows, max_iterations, factor):
        """llr_rows: float32 [n_cw, 648] in decoder order."""
        n = llr_rows.shape[0]
        assert llr_rows.dtype == torch.float32 and llr_rows.is_contiguous() and llr_rows.shape[1] == 648
        nb = (self.geo.ldpc_k + 7) // 8
        out = torch.empty((n, nb), dtype=torch.uint8, device=self.device)
        ok = torch.empty(n, dtype=torch.uint8, device=self.device)
        it = torch.empty(n, dtype=torch.int16, device=self.device)
        self._check(self.lib.ria_gpu_ldpc_decode_batch(self.h, _ptr(llr_rows), n, int(max_iterations), float(factor),
                                                       _ptr(out), _ptr(ok), _ptr(it), _stream_ptr()))
        return out, ok, it

    def ldpc_decode_robust(self, llr_rows):
        """robustDecodeSingleCW over a batch: llr_rows float32 [n_cw, 648] -> (bytes, ok, iterations, tries)"""
        n = llr_rows.shape[0]
        assert llr_rows.dtype == torch.float32 and llr_rows.is_contiguous() and llr_rows.shape[1] == 648
        nb = (self.geo.ldpc_k + 7) // 8
        out = torch.empty((n, nb), dtype=torch.uint8, device=self.device)
        ok = torch.empty(n, dtype=torch.uint8, device=self.device)
        it = torch.empty(n, dtype=torch.int16, device=self.device)
        tries = torch.empty(n, dtype=torch.uint8, device=self.device)
        self._check(self.lib.ria_gpu_ldpc_decode_robust_batch(self.h, _ptr(llr_rows), n, _ptr(out), _ptr(ok), _ptr(it),
                                                              _ptr(tries), _stream_ptr()))
        return out, ok, it, tries

    def ldpc_encode(self, info):
        """LDPCEncoder::encode on the host: info uint8 [n_cw, ceil(k/8)] -> coded uint8 [n_cw, 81]."""
        info = np.ascontiguousarray(info, np.uint8)
        out = np.zeros((info.shape[0], 81), np.uint8)
        self._check(self.lib.ria_gpu_ldpc_encode_host(self.h, info.ctypes.data, info.shape[0], out.ctypes.data))
        return out

    def make_frames(self, seed, first_seq, n):
        info = torch.empty((n, self.geo.info_bytes_per_frame), dtype=torch.uint8, device=self.device)
        self._check(self.lib.ria_gpu_make_frames(self.h, int(seed), int(first_seq), n, _ptr(info), _stream_ptr()))
        return info

    def tx(self, info, peak=0.8):
        n = info.shape[0]
        assert info.dtype == torch.uint8 and info.is_contiguous() and info.shape[1] == self.geo.info_bytes_per_frame
        s = torch.empty((n, self.geo.frame_samples), dtype=torch.float32, device=self.device)
        self._check(self.lib.ria_gpu_tx_batch(self.h, _ptr(info), n, float(peak), _ptr(s), _stream_ptr()))
        return s

    def encode_frames(self, info):
        """encodeFixedFrame alone: info uint8 [n, info_bytes] -> coded uint8 [n, 324] (channel interleaved)."""
        n = info.shape[0]
        assert info.dtype == torch.uint8 and info.is_contiguous() and info.shape[1] == self.geo.info_bytes_per_frame
        coded = torch.empty((n, 324), dtype=torch.uint8, device=self.device)
        self._check(self.lib.ria_gpu_encode_frames_batch(self.h, _ptr(info), n, _ptr(coded), _stream_ptr()))
        return coded

    def tx_coded(self, coded, peak=0.8):
        """The modulator on coded bytes (uint8 [n, 324], e.g. burst_interleave's output) -> samples [n, frame_samples]."""
        n = coded.shape[0]
        assert coded.dtype == torch.uint8 and coded.is_contiguous() and coded.shape[1] == 324
        s = torch.empty((n, self.geo.frame_samples), dtype=torch.float32, device=self.device)
        self._check(self.lib.ria_gpu_tx_coded_batch(self.h, _ptr(coded), n, float(peak), _ptr(s), _stream_ptr()))
        return s

    def channel_(self, samples, kind, snr_db, seed, first_frame=0):
        n = samples.shape[0]
        assert samples.dtype == torch.float32 and samples.is_contiguous()
        self._check(self.lib.ria_gpu_channel_batch(self.h, int(kind), float(snr_db), int(seed), int(first_frame),
                                                   _ptr(samples), n, _stream_ptr()))
        return samples

    ZC_RESULT = np.dtype([("detected", "<i4"), ("frame_type", "<i4"), ("start_sample", "<i4"), ("root_detected", "<i4"),
                          ("correlation", "<f4"), ("cfo_hz", "<f4"), ("snr_estimate", "<f4"), ("reserved", "<f4")])

    def sync_zc(self, buffers, threshold=0.3, root_mask=15, known_cfo=None):
        """ZCSync::detect over a batch: buffers float32 [n, buf_len] on the device -> structured array."""
        n, buf_len = buffers.shape
        assert buffers.dtype == torch.float32 and buffers.is_contiguous()
        out = torch.zeros((n, 32), dtype=torch.uint8, device=self.device)
        if known_cfo is not None:
            assert known_cfo.dtype == torch.float32 and known_cfo.numel() == n
        self._check(self.lib.ria_gpu_sync_zc_batch(self.h, _ptr(buffers), buf_len, buf_len, n, float(threshold),
                                                   int(root_mask), _ptr(known_cfo), _ptr(out), _stream_ptr()))
        return self._status_array(out, self.ZC_RESULT)

    def zc_preamble(self, root):
        out = np.zeros(4096, np.float32)
        n = self.lib.ria_gpu_zc_preamble(self.h, int(root), out.ctypes.data, len(out))
        if n < 0:
            raise capi.RiaError("zc_preamble: buffer too small")
        return out[:n].copy()

    CHIRP_RESULT = np.dtype([("success", "<i4"), ("up_chirp_start", "<i4"), ("down_chirp_start", "<i4"), ("cfo_hz", "<f4"),
                             ("up_correlation", "<f4"), ("down_correlation", "<f4"), ("reserved", "<i4", 2)])

    def sync_chirp(self, buffers, threshold=0.15):
        """ChirpSync::detectDualChirp over a batch: buffers float32 [n, buf_len] on the device -> structured array."""
        n, buf_len = buffers.shape
        assert buffers.dtype == torch.float32 and buffers.is_contiguous()
        out = torch.zeros((n, 32), dtype=torch.uint8, device=self.device)
        self._check(self.lib.ria_gpu_sync_chirp_batch(self.h, _ptr(buffers), buf_len, buf_len, n, float(threshold),
                                                      _ptr(out), _stream_ptr()))
        return self._status_array(out, self.CHIRP_RESULT)

    def chirp_preamble(self):
        out = np.zeros(60000, np.float32)
        n = self.lib.ria_gpu_chirp_preamble(self.h, out.ctypes.data, len(out))
        if n < 0:
            raise capi.RiaError("chirp_preamble: buffer too small")
        return out[:n].copy()

    LTS_RESULT = np.dtype([("detected", "<i4"), ("start_sample", "<i4"), ("correlation", "<f4"), ("cfo_hz", "<f4"),
                           ("burst_interleaved", "<i4"), ("reserved", "<i4", 3)])

    def sync_lts(self, buffers, known_cfo=None, threshold=0.5):
        """OFDMChirpWaveform::detectDataSync over a batch: buffers float32 [n, buf_len] on the device."""
        n, buf_len = buffers.shape
        assert buffers.dtype == torch.float32 and buffers.is_contiguous()
        out = torch.zeros((n, 32), dtype=torch.uint8, device=self.device)
        self._check(self.lib.ria_gpu_sync_lts_batch(self.h, _ptr(buffers), buf_len, buf_len, n, _ptr(known_cfo), float(threshold),
                                                    _ptr(out), _stream_ptr()))
        return self._status_array(out, self.LTS_RESULT)

    ACQ_PARAMS = np.dtype([("known_cfo_hz", "<f4"), ("detect_threshold", "<f4"), ("min_confidence", "<f4"), ("reserved0", "<u4"),
                           ("abs_base", "<u8"), ("reserved", "<u4", 2)])
    ACQ_RESULT = np.dtype([("detected", "<i4"), ("accepted", "<i4"), ("sync_start", "<i4"), ("frame_start", "<i4"),
                           ("correlation", "<f4"), ("cfo_hz", "<f4"), ("delta", "<i2"), ("candidates", "u1"),
                           ("burst_interleaved", "u1"), ("reserved", "<i4")])

    def acq_params(self, n, known_cfo=None, detect_threshold=0.15, min_confidence=None, abs_base=None):
        """ria_acq_params for n windows as a uint8 [n, 32] device tensor (scalars or one value per window)"""
        from .acquire import lts_min_confidence
        if min_confidence is None:
            min_confidence = lts_min_confidence(self.modulation)
        p = np.zeros(n, self.ACQ_PARAMS)
        p["known_cfo_hz"] = 0.0 if known_cfo is None else known_cfo
        p["detect_threshold"] = detect_threshold
        p["min_confidence"] = min_confidence
        p["abs_base"] = 0 if abs_base is None else abs_base
        return torch.from_numpy(p.view(np.uint8).reshape(n, 32)).to(self.device)

    def rx_acquire(self, windows, search_len, known_cfo=None, detect_threshold=0.15, min_confidence=None, abs_base=None,
                   flags=capi.DECODE_FULL, retry=True, want_demod_status=False, params=None):
        """Connected-mode OFDM data frames from capture windows (ria_gpu_rx_acquire_batch): LTS detection on the first
        search_len samples of each row of `windows` (float32 [n, window_len] on the device), the acceptance test,
        demodulation + decodeFixedFrame at the detected start and, where no codeword decodes, the reference's timing
        recovery at +-8 .. +-32 samples.  known_cfo / detect_threshold / min_confidence / abs_base: scalars or one value per
        window (min_confidence None: acquire.lts_min_confidence of the handle's modulation without fading or SNR hints).
        params: the ria_acq_params already on the device (acq_params), instead of the four values.
        Returns (info, decode_status, acq_result[, frame_status]); acq_result is a structured array (ACQ_RESULT)."""
        n, window_len = windows.shape
        assert windows.dtype == torch.float32 and windows.is_contiguous()
        if params is None:
            params = self.acq_params(n, known_cfo, detect_threshold, min_confidence, abs_base)
        assert params.dtype == torch.uint8 and params.shape == (n, 32) and params.is_contiguous()
        info = torch.empty((n, self.geo.info_bytes_per_frame), dtype=torch.uint8, device=self.device)
        st = torch.empty((n, 20), dtype=torch.uint8, device=self.device)
        acq = torch.empty((n, 32), dtype=torch.uint8, device=self.device)
        fst = torch.empty((n, 32), dtype=torch.uint8, device=self.device) if want_demod_status else None
        fl = int(flags) | (0 if retry else capi.ACQ_NO_TIMING_RETRY)
        self._check(self.lib.ria_gpu_rx_acquire_batch(self.h, _ptr(windows), window_len, int(search_len), window_len, n, _ptr(params), fl,
                                                      _ptr(info), _ptr(st), _ptr(acq), _ptr(fst), _stream_ptr()))
        res = self._status_array(acq, self.ACQ_RESULT)
        return (info, st, res, fst) if want_demod_status else (info, st, res)

    # ---- frames of any length and the control hypothesis
    CONTROL_RESULT = np.dtype([("process_ok", "u1"), ("cw_ok", "u1"), ("magic", "u1"), ("header_valid", "u1"), ("total_cw", "u1"),
                               ("frame_type", "u1"), ("success", "u1"), ("tries", "u1"), ("seq", "<u2"), ("iterations", "<u2"),
                               ("n_llr", "<i4"), ("tried", "u1"), ("reserved0", "u1", 3), ("reserved", "<i4", 3)])

    def var_frame_samples(self, coded_bytes):
        """samples of a frame of coded_bytes coded bytes (1..324) at this engine's modulation"""
        n = self.lib.ria_gpu_var_frame_samples(self.h, int(coded_bytes))
        if n < 0:
            self._check(n)
        return n

    def control_frame_samples(self, data_engine):
        """getOFDMControlFrameSamples: the span the receiver tries the control hypothesis on; self is the control engine"""
        n = self.lib.ria_gpu_control_frame_samples(self.h, data_engine.h)
        if n < 0:
            self._check(n)
        return n

    def tx_coded_var(self, coded, peak=0.8, out_stride=None):
        """The modulator on any number of coded bytes: coded uint8 [n, 1..324] -> samples [n, out_stride or the frame's length]"""
        n, nb = coded.shape
        assert coded.dtype == torch.uint8 and coded.is_contiguous()
        ns = self.var_frame_samples(nb)
        stride = ns if out_stride is None else int(out_stride)
        s = torch.zeros((n, stride), dtype=torch.float32, device=self.device)
        self._check(self.lib.ria_gpu_tx_coded_var_batch(self.h, _ptr(coded), nb, n, float(peak), _ptr(s), stride, _stream_ptr()))
        return s

    def _spans_in(self, samples, offsets, n_samples):
        assert samples.dtype == torch.float32 and samples.is_contiguous()
        if offsets is None:
            assert samples.dim() == 2 and samples.shape[1] == n_samples
            return samples.shape[0], None
        off = np.ascontiguousarray(offsets, np.uint64)
        assert off.size == 0 or int(off.max()) + n_samples <= samples.numel(), "span runs past the capture"
        return len(off), torch.from_numpy(off.view(np.int64)).to(self.device)

    def demod_var(self, samples, n_samples=None, cfo_hz=None, abs_pos=None, flags=None, offsets=None):
        """process() + getSoftBits() on spans of n_samples samples: float32 [n, n_samples] rows, or one capture + offsets
        -> (llr [n, (n_samples // 1152 - 2) * bits_per_symbol], status)"""
        n_samples = samples.shape[1] if n_samples is None else int(n_samples)
        n, off = self._spans_in(samples, offsets, n_samples)
        row = max(0, n_samples // 1152 - 2) * self.geo.bits_per_symbol
        llr = torch.zeros((n, max(row, 1)), dtype=torch.float32, device=self.device)
        st = torch.zeros((n, 32), dtype=torch.uint8, device=self.device)
        meta = self._meta(n, cfo_hz, abs_pos, flags)
        self._check(self.lib.ria_gpu_demod_var_batch(self.h, _ptr(samples), _ptr(off), _ptr(meta), n, n_samples, _ptr(llr),
                                                     llr.shape[1], _ptr(st), _stream_ptr()))
        return llr[:, :row], st

    def demod_var_host(self, samples, cfo_hz=0.0, abs_pos=0, flags=0):
        """One span from host memory (ria_gpu_demod_var_host, the IWaveform adaptor's path for spans shorter than a frame):
        samples float32 numpy [n_samples] -> (llr numpy, status structured scalar)"""
        x = np.ascontiguousarray(samples, np.float32)
        row = max(0, len(x) // 1152 - 2) * self.geo.bits_per_symbol
        llr = np.zeros(max(row, 1), np.float32)
        meta = capi.FrameMeta(float(cfo_hz), int(flags), int(abs_pos))
        st = np.zeros(1, self.FRAME_STATUS)
        self._check(self.lib.ria_gpu_demod_var_host(self.h, x.ctypes.data, len(x), C.addressof(meta), llr.ctypes.data, row, st.ctypes.data))
        return llr[:row], st[0]

    def rx_control(self, samples, n_samples=None, cfo_hz=None, abs_pos=None, flags=None, offsets=None):
        """The control hypothesis on pre-synced spans (ria_gpu_rx_control_batch; a DQPSK R1/4 engine):
        -> (frame bytes uint8 [n, 20], result structured array (CONTROL_RESULT), frame status)"""
        n_samples = samples.shape[1] if n_samples is None else int(n_samples)
        n, off = self._spans_in(samples, offsets, n_samples)
        frames = torch.empty((n, 20), dtype=torch.uint8, device=self.device)
        res = torch.empty((n, 32), dtype=torch.uint8, device=self.device)
        st = torch.empty((n, 32), dtype=torch.uint8, device=self.device)
        meta = self._meta(n, cfo_hz, abs_pos, flags)
        self._check(self.lib.ria_gpu_rx_control_batch(self.h, _ptr(samples), _ptr(off), _ptr(meta), n, n_samples, _ptr(frames),
                                                      _ptr(res), _ptr(st), _stream_ptr()))
        return frames, self._status_array(res, self.CONTROL_RESULT), st

    def control_acquire(self, windows, search_len, n_samples, known_cfo=None, detect_threshold=0.15, min_confidence=None,
                        abs_base=None, interleave=False, params=None, want_device_result=False):
        """The control hypothesis from capture windows (ria_gpu_control_acquire_batch): rx_acquire's detection and acceptance,
        then rx_control on the span of n_samples at the detected start.  min_confidence None: that of the DATA profile has to be
        passed by the caller; here it defaults to this engine's (DQPSK).  interleave: RIA_BURST_INTERLEAVE (marked windows are
        left to the burst path).  Returns (frame bytes [n, 20], result (CONTROL_RESULT), acq (ACQ_RESULT), frame status[,
        the result rows as a uint8 [n, 32] device tensor])."""
        n, window_len = windows.shape
        assert windows.dtype == torch.float32 and windows.is_contiguous()
        if params is None:
            params = self.acq_params(n, known_cfo, detect_threshold, min_confidence, abs_base)
        assert params.dtype == torch.uint8 and params.shape == (n, 32) and params.is_contiguous()
        frames = torch.empty((n, 20), dtype=torch.uint8, device=self.device)
        res = torch.empty((n, 32), dtype=torch.uint8, device=self.device)
        acq = torch.empty((n, 32), dtype=torch.uint8, device=self.device)
        st = torch.empty((n, 32), dtype=torch.uint8, device=self.device)
        self._check(self.lib.ria_gpu_control_acquire_batch(self.h, _ptr(windows), window_len, int(search_len), window_len, n,
                                                           int(n_samples), _ptr(params), capi.BURST_INTERLEAVE if interleave else 0,
                                                           _ptr(frames), _ptr(res), _ptr(acq), _ptr(st), _stream_ptr()))
        out = (frames, self._status_array(res, self.CONTROL_RESULT), self._status_array(acq, self.ACQ_RESULT), st)
        return out + (res,) if want_device_result else out

    WINDOW_RESULT = np.dtype([("frame", DFRAME_RESULT), ("outcome", "u1"), ("peek", "u1"), ("pending_total_cw", "u1"), ("small_frame", "u1"),
                              ("tries_peek_r14", "u1"), ("tries_peek_rate", "u1"), ("tries_small_r14", "u1"), ("tries_small_rate", "u1"),
                              ("frame_len", "<i4"), ("next_pos", "<i4"), ("need_samples", "<i4"), ("sync_cfo_hz", "<f4"),
                              ("peek_cfo_hz", "<f4"), ("fading_index", "<f4")])

    def window_frame_row(self):
        """bytes of one frame row of rx_window: decodeFrame's row for a whole frame's soft bits"""
        return max(4, self.geo.llrs_per_frame // 648) * self.geo.bytes_per_codeword

    def rx_window(self, control_engine, windows, search_len, known_cfo=None, detect_threshold=0.15, min_confidence=None, abs_base=None,
                  flags=capi.DECODE_FULL, interleave=False, retry=True, params=None):
        """One connected-mode OFDM-CHIRP window per row of `windows` (float32 [n, window_len] on the device), as
        StreamingDecoder handles it (ria_gpu_rx_window_batch): detection and acceptance, the control hypothesis on
        control_engine (DQPSK R1/4), the peek with this engine's profile and its CFO feedback, the escalation to the frame the
        CW0 header announces, decodeFrame, small-frame recovery, timing recovery and the consumed samples.  self is the data
        engine.  Returns (frame bytes uint8 [n, window_frame_row()], result (WINDOW_RESULT), acq (ACQ_RESULT), control result
        (CONTROL_RESULT), frame status of the reported span)."""
        n, window_len = windows.shape
        assert windows.dtype == torch.float32 and windows.is_contiguous()
        if params is None:
            params = self.acq_params(n, known_cfo, detect_threshold, min_confidence, abs_base)
        assert params.dtype == torch.uint8 and params.shape == (n, 32) and params.is_contiguous()
        row = self.window_frame_row()
        frames = torch.empty((n, row), dtype=torch.uint8, device=self.device)
        res = torch.empty((n, 64), dtype=torch.uint8, device=self.device)
        acq = torch.empty((n, 32), dtype=torch.uint8, device=self.device)
        cres = torch.empty((n, 32), dtype=torch.uint8, device=self.device)
        st = torch.empty((n, 32), dtype=torch.uint8, device=self.device)
        fl = int(flags) | (capi.BURST_INTERLEAVE if interleave else 0) | (0 if retry else capi.ACQ_NO_TIMING_RETRY)
        self._check(self.lib.ria_gpu_rx_window_batch(control_engine.h, self.h, _ptr(windows), window_len, int(search_len), window_len, n,
                                                     _ptr(params), fl, _ptr(frames), row, _ptr(res), _ptr(acq), _ptr(cres), _ptr(st),
                                                     _stream_ptr()))
        return (frames, self._status_array(res, self.WINDOW_RESULT), self._status_array(acq, self.ACQ_RESULT),
                self._status_array(cres, self.CONTROL_RESULT), st)

    BURST_RESULT = np.dtype([("detected", "<i4"), ("accepted", "<i4"), ("sync_start", "<i4"), ("frame_start", "<i4"),
                             ("correlation", "<f4"), ("cfo_hz", "<f4"), ("delta", "<i2"), ("candidates", "u1"),
                             ("burst_interleaved", "u1"), ("mode", "u1"), ("frames", "u1"), ("frames_decoded", "u1"),
                             ("stop", "u1"), ("reserved", "<i4", 8)])

    def rx_burst(self, windows, search_len, group_size=4, known_cfo=None, detect_threshold=0.15, min_confidence=None, abs_base=None,
                 flags=capi.DECODE_FULL, interleave=True, continuation=True, retry=True, window_len=None, sync=True):
        """Burst groups and burst continuation from capture windows (ria_gpu_rx_burst_batch): what rx_acquire does for the
        first frame of each row of `windows` (float32 [n, stride] on the device; window_len <= stride samples of a row are
        the window), then, with `interleave`, a marked window's group of group_size physical frames (energy gate, CFO chain,
        burst de-interleave, decodeFixedFrame per logical frame) and, for every other accepted window, up to 8 continuation
        blocks behind a successfully decoded data frame (`continuation`).  Parameters as rx_acquire.
        Returns a dict: info uint8 [n, 9, info_bytes], decode_status / frame_status structured [n, 9], cfo_used / rms
        float32 [n, 9], result structured [n] (BURST_RESULT).  sync=False leaves the arrays on the device (torch tensors,
        raw bytes for the structured ones) and does not wait."""
        from .acquire import lts_min_confidence
        n, stride = windows.shape
        window_len = stride if window_len is None else int(window_len)
        assert windows.dtype == torch.float32 and windows.is_contiguous()
        if min_confidence is None:
            min_confidence = lts_min_confidence(self.modulation)
        p = np.zeros(n, self.ACQ_PARAMS)
        p["known_cfo_hz"] = 0.0 if known_cfo is None else known_cfo
        p["detect_threshold"] = detect_threshold
        p["min_confidence"] = min_confidence
        p["abs_base"] = 0 if abs_base is None else abs_base
        params = torch.from_numpy(p.view(np.uint8).reshape(n, 32)).to(self.device)
        S = capi.BURST_MAX_FRAMES
        info = torch.empty((n, S, self.geo.info_bytes_per_frame), dtype=torch.uint8, device=self.device)
        st = torch.empty((n, S, 20), dtype=torch.uint8, device=self.device)
        res = torch.empty((n, 64), dtype=torch.uint8, device=self.device)
        fst = torch.empty((n, S, 32), dtype=torch.uint8, device=self.device)
        cfo = torch.empty((n, S), dtype=torch.float32, device=self.device)
        rms = torch.empty((n, S), dtype=torch.float32, device=self.device)
        fl = int(flags) | (0 if retry else capi.ACQ_NO_TIMING_RETRY) | (capi.BURST_INTERLEAVE if interleave else 0) | \
            (0 if continuation else capi.BURST_NO_CONTINUE)
        self._check(self.lib.ria_gpu_rx_burst_batch(self.h, _ptr(windows), stride, int(search_len), window_len, n, int(group_size),
                                                    _ptr(params), fl, _ptr(info), _ptr(st), _ptr(res), _ptr(fst), _ptr(cfo), _ptr(rms),
                                                    _stream_ptr()))
        if not sync:
            return dict(info=info, decode_status=st, result=res, frame_status=fst, cfo_used=cfo, rms=rms)
        torch.cuda.synchronize()
        return dict(info=info.cpu().numpy(), decode_status=self._status_array(st, self.DECODE_STATUS).reshape(n, S),
                    result=self._status_array(res, self.BURST_RESULT), frame_status=self._status_array(fst, self.FRAME_STATUS).reshape(n, S),
                    cfo_used=cfo.cpu().numpy(), rms=rms.cpu().numpy())

    COX_RESULT = np.dtype([("found", "<i4"), ("start_sample", "<i4"), ("cfo_hz", "<f4"), ("noise_floor", "<f4"),
                           ("sts_position", "<i4"), ("reserved", "<i4", 3)])

    def sync_cox(self, buffers, threshold=0.8, noise_floor=None):
        """OFDMDemodulator::searchForSync (Schmidl-Cox, OFDM-COX waveform) over a batch: buffers float32
        [n, buf_len] on the device; noise_floor float32 [n] = the demodulator's tracker before the call."""
        n, buf_len = buffers.shape
        assert buffers.dtype == torch.float32 and buffers.is_contiguous()
        out = torch.zeros((n, 32), dtype=torch.uint8, device=self.device)
        self._check(self.lib.ria_gpu_sync_cox_batch(self.h, _ptr(buffers), buf_len, buf_len, n, float(threshold), _ptr(noise_floor),
                                                    _ptr(out), _stream_ptr()))
        return self._status_array(out, self.COX_RESULT)

    def cox_preamble(self):
        out = np.zeros(10000, np.float32)
        n = self.lib.ria_gpu_cox_preamble(self.h, out.ctypes.data, len(out))
        if n < 0:
            raise capi.RiaError("cox_preamble: buffer too small")
        return out[:n].copy()

    MCDPSK_STATUS = np.dtype([("cfo_hz", "<f4"), ("fading_index", "<f4"), ("freq_fading_index", "<f4"),
                              ("temporal_fading_index", "<f4"), ("training_cfo_residual", "<f4"), ("n_llr", "<i4"),
                              ("valid_symbols", "<i4"), ("reserved", "<i4")])

    def mcdpsk_demod(self, frames, carriers=10, bits_per_symbol=1, spreading=1, cfo_hz=None, phase0=None):
        """MC-DPSK demodulator over a batch: frames float32 [n, (9 + symbols)*512] -> (llr [n, n_llr], status)."""
        n, fs = frames.shape
        assert frames.dtype == torch.float32 and frames.is_contiguous()
        cfg = capi.McdpskConfig(carriers, bits_per_symbol, spreading, 0)
        n_llr = max(1, ((fs - 9 * 512) // 512) // spreading) * carriers * bits_per_symbol
        llr = torch.empty((n, n_llr), dtype=torch.float32, device=self.device)
        st = torch.zeros((n, 32), dtype=torch.uint8, device=self.device)
        self._check(self.lib.ria_gpu_mcdpsk_demod_batch(self.h, C.byref(cfg), _ptr(frames), fs, fs, n, _ptr(cfo_hz), _ptr(phase0),
                                                        _ptr(llr), n_llr, _ptr(st), _stream_ptr()))
        return llr, self._status_array(st, self.MCDPSK_STATUS)

    MCACQ_PARAMS = ACQ_PARAMS
    MCACQ_RESULT = np.dtype([("detected", "<i4"), ("accepted", "<i4"), ("sync_start", "<i4"), ("frame_start", "<i4"),
                             ("correlation", "<f4"), ("cfo_hz", "<f4"), ("fading_index", "<f4"), ("delta", "<i2"),
                             ("modulation", "u1"), ("candidates", "u1"), ("success", "u1"), ("codewords_ok", "u1"),
                             ("codewords_failed", "u1"), ("frame_type", "u1"), ("header_total_cw", "<i4"),
                             ("frame_bytes", "<i4"), ("n_llr", "<i4"), ("reserved", "<i4", 4)])

    def mcdpsk_acquire(self, windows, search_len, frame_cw, carriers=10, modulation="DBPSK", spreading=1, sync="chirp",
                       disconnected=None, known_cfo=None, detect_threshold=None, min_confidence=None, abs_base=None, retry=True,
                       want_llr=False, chase=None, cache_id=None, now_ms=None, harq_entry=False, channel_interleave=False,
                       interleaver_bits=None):
        """MC-DPSK frames from capture windows (ria_gpu_mcdpsk_acquire_batch): ZC ("zc") or dual-chirp ("chirp") detection
        on the first search_len samples of each row of `windows` (float32 [n, window_len] on the device), the acceptance
        test, demodulation + decodeMCDPSKFrame at R1/4 and, when `disconnected` (default: chirp), the handshake fallbacks.
        The handle must be R1/4.  known_cfo / detect_threshold / min_confidence / abs_base: scalars or one value per window
        (defaults: 0, the reference's 0.2 ZC / 0.15 chirp, acquire.zc_min_confidence(0) for ZC and 0 for chirp).
        chase: a ChasePool routes the call to ria_gpu_mcdpsk_acquire_harq_batch; window b then uses cache cache_id[b] (default
        b, -1 = off) at time now_ms (scalar or one per window, default 0).  harq_entry: use that entry point without a pool too
        (the same outputs as the plain call, plus an all-zero harq array).
        channel_interleave: the link negotiated MC-DPSK channel interleaving (ria_gpu_mcdpsk_acquire_ci_batch, with or
        without a pool); interleaver_bits is the width of the receiver's interleaver (None: carriers x bits of the primary
        modulation; a receiver configured by setMode alone has carriers x 2).  The result then carries
        two more fields, cw0_deinterleaved and ci_tried, of the reported candidate.
        Returns (frames uint8 [n, 40 * frame_cw], acq_result structured array (MCACQ_RESULT)[, llr float32 [n, stride]]
        [, harq result structured array (HARQ_RESULT) when chase is given])."""
        from .acquire import zc_min_confidence
        n, window_len = windows.shape
        assert windows.dtype == torch.float32 and windows.is_contiguous()
        chirp = {"chirp": True, "zc": False}[sync]
        if disconnected is None:
            disconnected = chirp
        bps = {"DBPSK": 1, "DQPSK": 2}[modulation] if isinstance(modulation, str) else int(modulation)
        p = np.zeros(n, self.MCACQ_PARAMS)
        p["known_cfo_hz"] = 0.0 if known_cfo is None else known_cfo
        p["detect_threshold"] = (0.15 if chirp else 0.2) if detect_threshold is None else detect_threshold
        p["min_confidence"] = (0.0 if chirp else zc_min_confidence(0)) if min_confidence is None else min_confidence
        p["abs_base"] = 0 if abs_base is None else abs_base
        params = torch.from_numpy(p.view(np.uint8).reshape(n, 32)).to(self.device)
        fl = (capi.MACQ_SYNC_CHIRP if chirp else 0) | (capi.MACQ_DISCONNECTED if disconnected else 0) | (0 if retry else capi.MACQ_NO_RETRY)
        frames = torch.empty((n, capi.macq_frame_bytes(frame_cw)), dtype=torch.uint8, device=self.device)
        acq = torch.empty((n, 64), dtype=torch.uint8, device=self.device)
        llr, stride = None, 0
        if want_llr:
            stride = frame_cw * -(-648 // (carriers * bps)) * carriers * 2        # room for either modulation
            llr = torch.empty((n, stride), dtype=torch.float32, device=self.device)
        cfg = capi.McdpskConfig(carriers, bps, spreading, 0)
        if chase is None and not harq_entry and not channel_interleave:
            self._check(self.lib.ria_gpu_mcdpsk_acquire_batch(self.h, C.byref(cfg), _ptr(windows), window_len, int(search_len), window_len, n,
                                                              int(frame_cw), _ptr(params), fl, _ptr(frames), _ptr(acq), _ptr(llr), stride,
                                                              _stream_ptr()))
            res = self._status_array(acq, self.MCACQ_RESULT)
            return (frames, res, llr) if want_llr else (frames, res)
        ids, now, harq = self._harq_in(n, cache_id, now_ms)
        if channel_interleave:
            bits = carriers * bps if interleaver_bits is None else int(interleaver_bits)
            self._check(self.lib.ria_gpu_mcdpsk_acquire_ci_batch(self.h, C.byref(cfg), _ptr(windows), window_len, int(search_len), window_len, n,
                                                                 int(frame_cw), _ptr(params), fl | capi.MACQ_CHANNEL_INTERLEAVE, _ptr(frames), _ptr(acq),
                                                                 _ptr(llr), stride, chase.p if chase is not None else None, _ptr(ids), _ptr(now),
                                                                 _ptr(harq), bits, _stream_ptr()))
            res = self._status_array(acq, self.MCACQ_RESULT)
            res = self._ci_fields(res, res["reserved"][:, 0])
            out = (frames, res, llr) if want_llr else (frames, res)
            return out + (self._status_array(harq, self.HARQ_RESULT),) if (chase is not None or harq_entry) else out
        self._check(self.lib.ria_gpu_mcdpsk_acquire_harq_batch(self.h, C.byref(cfg), _ptr(windows), window_len, int(search_len), window_len, n,
                                                               int(frame_cw), _ptr(params), fl, _ptr(frames), _ptr(acq), _ptr(llr), stride,
                                                               chase.p if chase is not None else None, _ptr(ids), _ptr(now), _ptr(harq),
                                                               _stream_ptr()))
        res = self._status_array(acq, self.MCACQ_RESULT)
        hq = self._status_array(harq, self.HARQ_RESULT)
        return (frames, res, llr, hq) if want_llr else (frames, res, hq)

    MCWIN_PARAMS = np.dtype([("known_cfo_hz", "<f4"), ("detect_threshold", "<f4"), ("min_confidence", "<f4"), ("pending_total_cw", "<u4"),
                             ("abs_base", "<u8"), ("first_avail", "<u4"), ("last_decoded_sync", "<i4")])
    MCWIN_RESULT = np.dtype([("outcome", "<i4"), ("peek", "<i4"), ("next_pos", "<i4"), ("need_samples", "<i4"), ("pending_total_cw", "<i4"),
                             ("frame_len", "<i4"), ("passes", "<i4"), ("peek_total_cw", "<i4"), ("training_rms", "<f4"), ("rms", "<f4"),
                             ("last_decoded_sync", "<i4"), ("deliver", "u1"), ("is_ping", "u1"), ("peek_tries", "u1"), ("reserved0", "u1"),
                             ("reserved", "<i4", 4)])
    MCWIN_FRAME_ROW = 320    # RIA_MACQ_FRAME_BYTES(8)

    def mcdpsk_window(self, windows, search_len, carriers=10, modulation="DBPSK", spreading=1, sync="chirp", disconnected=None,
                      known_cfo=None, detect_threshold=None, min_confidence=None, abs_base=None, retry=True, want_llr=False,
                      chase=None, cache_id=None, now_ms=None, channel_interleave=False, interleaver_bits=None,
                      pending_total_cw=None, first_avail=None, last_decoded_sync=None):
        """One MC-DPSK window the way StreamingDecoder::decodeCurrentFrame handles it (ria_gpu_mcdpsk_window_batch): detection
        and acceptance, anti-replay, the PING energy test (disconnected), the CW0 peek and its escalation, decodeMCDPSKFrame on
        the last pass's soft bits and the handshake fallbacks.  Arguments as mcdpsk_acquire, without frame_cw; per window
        (scalars or one value each): pending_total_cw (default 0: a fresh sync), first_avail (default 0: a whole 1-codeword
        span), last_decoded_sync (default None: no anti-replay position).  chase: a ChasePool; window b uses cache cache_id[b]
        (default b, -1 = off) at now_ms.  channel_interleave / interleaver_bits as in mcdpsk_acquire.
        Returns (frames uint8 [n, 320], result (MCWIN_RESULT), acq (MCACQ_RESULT with cw0_deinterleaved and ci_tried),
        harq (HARQ_RESULT)[, llr float32 [n, stride]])."""
        from .acquire import zc_min_confidence
        n, window_len = windows.shape
        assert windows.dtype == torch.float32 and windows.is_contiguous()
        chirp = {"chirp": True, "zc": False}[sync]
        if disconnected is None:
            disconnected = chirp
        bps = {"DBPSK": 1, "DQPSK": 2}[modulation] if isinstance(modulation, str) else int(modulation)
        p = np.zeros(n, self.MCWIN_PARAMS)
        p["known_cfo_hz"] = 0.0 if known_cfo is None else known_cfo
        p["detect_threshold"] = (0.15 if chirp else 0.2) if detect_threshold is None else detect_threshold
        p["min_confidence"] = (0.0 if chirp else zc_min_confidence(0)) if min_confidence is None else min_confidence
        p["abs_base"] = 0 if abs_base is None else abs_base
        p["pending_total_cw"] = 0 if pending_total_cw is None else pending_total_cw
        p["first_avail"] = 0 if first_avail is None else first_avail
        p["last_decoded_sync"] = capi.MWIN_NO_LAST_SYNC if last_decoded_sync is None else last_decoded_sync
        params = torch.from_numpy(p.view(np.uint8).reshape(n, 32)).to(self.device)
        fl = (capi.MACQ_SYNC_CHIRP if chirp else 0) | (capi.MACQ_DISCONNECTED if disconnected else 0) | (0 if retry else capi.MACQ_NO_RETRY) | \
             (capi.MACQ_CHANNEL_INTERLEAVE if channel_interleave else 0)
        row = self.MCWIN_FRAME_ROW
        frames = torch.empty((n, row), dtype=torch.uint8, device=self.device)
        res = torch.empty((n, 64), dtype=torch.uint8, device=self.device)
        acq = torch.empty((n, 64), dtype=torch.uint8, device=self.device)
        llr, stride = None, 0
        if want_llr:
            cw_samples = -(-648 // (carriers * bps)) * 512 * spreading
            top = max(1, min(8, (window_len - 9 * 512) // cw_samples))
            stride = top * -(-648 // (carriers * bps)) * carriers * 2
            llr = torch.empty((n, stride), dtype=torch.float32, device=self.device)
        cfg = capi.McdpskConfig(carriers, bps, spreading, 0)
        ids, now, harq = self._harq_in(n, cache_id, now_ms)
        bits = (carriers * bps if interleaver_bits is None else int(interleaver_bits)) if channel_interleave else 0
        self._check(self.lib.ria_gpu_mcdpsk_window_batch(self.h, C.byref(cfg), _ptr(windows), window_len, int(search_len), window_len, n,
                                                         _ptr(params), fl, _ptr(frames), row, _ptr(res), _ptr(acq), _ptr(llr), stride,
                                                         chase.p if chase is not None else None, _ptr(ids), _ptr(now), _ptr(harq), bits,
                                                         _stream_ptr()))
        a = self._status_array(acq, self.MCACQ_RESULT)
        a = self._ci_fields(a, a["reserved"][:, 0])
        out = (frames, self._status_array(res, self.MCWIN_RESULT), a, self._status_array(harq, self.HARQ_RESULT))
        return out + (llr,) if want_llr else out

    @staticmethod
    def _ci_fields(res, bits):
        """res with the two channel-interleaving bits of its reserved word as fields of their own"""
        out = np.zeros(res.shape, np.dtype(res.dtype.descr + [("cw0_deinterleaved", "u1"), ("ci_tried", "u1")]))
        for f in res.dtype.names:
            out[f] = res[f]
        out["cw0_deinterleaved"] = np.asarray(bits) & 1
        out["ci_tried"] = (np.asarray(bits) >> 1) & 1
        return out

    SEARCH_STATE = np.dtype([("correlation_pos", "<i4"), ("fed", "<i4"), ("noise_floor", "<f4"), ("reject_streak", "<i4"),
                             ("last_cfo_hz", "<f4"), ("fading_hint", "<f4"), ("snr_hint", "<f4"), ("last_decoded_sync_pos", "<i4")])
    SEARCH_RESULT = np.dtype([("outcome", "<i4"), ("search_start", "<i4"), ("search_len", "<i4"), ("sync_position", "<i4"),
                              ("abs_position", "<i8"), ("correlation", "<f4"), ("known_cfo_hz", "<f4"), ("sync_cfo_hz", "<f4"),
                              ("sync_snr_db", "<f4"), ("detect_threshold", "<f4"), ("min_confidence", "<f4"), ("weak_accept", "<i4"),
                              ("marker", "<i4"), ("root", "<i4"), ("invocations", "<u4"), ("waits", "<u4"), ("rms_skips", "<u4"),
                              ("detector_runs", "<u4"), ("rejects", "<u4"), ("near_misses", "<u4"), ("weak_accepts", "<u4"),
                              ("replays", "<u4"), ("catchups_moderate", "<u4"), ("catchups_severe", "<u4"), ("reserved0", "<u4"), ("reserved1", "<u4"), ("reserved2", "<u4")])

    @classmethod
    def search_state(cls, n, fed=0):
        """n fresh decoder states (SEARCH_STATE): cursor 0, `fed` samples arrived, noise floor 0.001, no decoded position"""
        s = np.zeros(n, cls.SEARCH_STATE)
        s["fed"] = fed
        s["noise_floor"] = np.float32(0.001)
        s["last_decoded_sync_pos"] = capi.SEARCH_NO_LAST_SYNC
        return s

    def set_search_chunk(self, streams):
        """search() runs the detector on at most this many streams at a time; 0 = as many as its 256 MiB workspace holds"""
        self._check(self.lib.ria_gpu_set_option(self.h, capi.OPT_SEARCH_CHUNK, int(streams)))

    def search(self, captures, capture_len, state, mode, feed_step=0, max_invocations=1 << 20, connected=False,
               carriers=10, modulation="DBPSK", spreading=1):
        """StreamingDecoder::searchForSync for one capture per row of `captures` (float32 [n, stride] on the device;
        ria_gpu_search_batch): each stream is walked from its state's cursor to its next accepted sync.  capture_len: samples
        of each stream (scalar or one each, <= 959 999); state: SEARCH_STATE records (search_state()); mode: "OFDM_LTS" (the
        modulation class is this engine's), "MCDPSK_ZC" or "MCDPSK_CHIRP" (connected=True: the connected weak profile); feed_step
        samples arrive after every invocation (0: the recording is all there).  carriers / modulation / spreading: the MC-DPSK
        configuration of the two MC-DPSK modes.  Returns (result (SEARCH_RESULT), state (SEARCH_STATE))."""
        n, stride = captures.shape
        assert captures.dtype == torch.float32 and captures.is_contiguous()
        m = capi.SEARCH_MODE[mode] if isinstance(mode, str) else int(mode)
        lens = np.empty(n, np.int32)
        lens[:] = capture_len
        st = np.ascontiguousarray(state, self.SEARCH_STATE)
        assert st.shape == (n,)
        lens_d = torch.from_numpy(lens).to(self.device)
        st_d = torch.from_numpy(st.view(np.uint8).reshape(n, 32).copy()).to(self.device)
        res_d = torch.empty((n, 112), dtype=torch.uint8, device=self.device)
        cfg = None
        if m != capi.SEARCH_MODE["OFDM_LTS"]:
            bps = {"DBPSK": 1, "DQPSK": 2}[modulation] if isinstance(modulation, str) else int(modulation)
            cfg = C.byref(capi.McdpskConfig(carriers, bps, spreading, 0))
        self._check(self.lib.ria_gpu_search_batch(self.h, m, capi.SEARCH_CONNECTED if connected else 0, cfg, _ptr(captures), stride, _ptr(lens_d), n,
                                                  _ptr(st_d), int(feed_step), int(max_invocations), _ptr(res_d), _stream_ptr()))
        return self._status_array(res_d, self.SEARCH_RESULT), self._status_array(st_d, self.SEARCH_STATE)

    RING_STATE = np.dtype([("total_fed", "<i8"), ("correlation_pos", "<i4"), ("reject_streak", "<i4"), ("noise_floor", "<f4"),
                           ("last_cfo_hz", "<f4"), ("fading_hint", "<f4"), ("snr_hint", "<f4"), ("last_decoded_sync_pos", "<i4"),
                           ("overflow_events", "<u4"), ("overflow_dropped", "<u8")])
    RING_SEARCH_RESULT = np.dtype(SEARCH_RESULT.descr + [("abs_search_start", "<i8"), ("overflow_dropped", "<u8"), ("overflows", "<u4"),
                                                         ("drift_snaps", "<u4"), ("cursor_inits", "<u4"), ("span_wraps", "<u4")])

    @classmethod
    def ring_state(cls, n, total_fed=0):
        """n fresh decoder states (RING_STATE): cursor 0, `total_fed` samples arrived, noise floor 0.001, no decoded position"""
        s = np.zeros(n, cls.RING_STATE)
        s["total_fed"] = total_fed
        s["noise_floor"] = np.float32(0.001)
        s["last_decoded_sync_pos"] = capi.SEARCH_NO_LAST_SYNC
        return s

    def search_ring(self, captures, capture_len, state, mode, feed_step=0, max_invocations=1 << 20, connected=False,
                    carriers=10, modulation="DBPSK", spreading=1):
        """search() for captures of any length up to 2^31 - 1 - 960 000 samples (ria_gpu_search_ring_batch): the decoder's
        960 000-sample ring buffer wraps, with feedAudio's drift guard and overflow drop.  state: RING_STATE records
        (ring_state()), whose cursor and last decoded position are ring indices.  Other arguments as search().  Returns
        (result (RING_SEARCH_RESULT), state (RING_STATE))."""
        n, stride = captures.shape
        assert captures.dtype == torch.float32 and captures.is_contiguous()
        m = capi.SEARCH_MODE[mode] if isinstance(mode, str) else int(mode)
        lens = np.empty(n, np.int32)
        lens[:] = capture_len
        st = np.ascontiguousarray(state, self.RING_STATE)
        assert st.shape == (n,)
        lens_d = torch.from_numpy(lens).to(self.device)
        st_d = torch.from_numpy(st.view(np.uint8).reshape(n, 48).copy()).to(self.device)
        res_d = torch.empty((n, 144), dtype=torch.uint8, device=self.device)
        cfg = None
        if m != capi.SEARCH_MODE["OFDM_LTS"]:
            bps = {"DBPSK": 1, "DQPSK": 2}[modulation] if isinstance(modulation, str) else int(modulation)
            cfg = C.byref(capi.McdpskConfig(carriers, bps, spreading, 0))
        self._check(self.lib.ria_gpu_search_ring_batch(self.h, m, capi.SEARCH_CONNECTED if connected else 0, cfg, _ptr(captures), stride, _ptr(lens_d), n,
                                                       _ptr(st_d), int(feed_step), int(max_invocations), _ptr(res_d), _stream_ptr()))
        return self._status_array(res_d, self.RING_SEARCH_RESULT), self._status_array(st_d, self.RING_STATE)

    STREAM_EVENT = np.dtype([("sync_position", "<i4"), ("search_start", "<i4"), ("window_len", "<i4"), ("outcome", "<i4"), ("next_pos", "<i4"),
                             ("frame_bytes", "<i4"), ("need_samples", "<i4"), ("pending_total_cw", "<i4"), ("delivered", "u1"), ("success", "u1"),
                             ("codewords_ok", "u1"), ("codewords_failed", "u1"), ("frame_type", "u1"), ("reserved0", "u1", 3),
                             ("correlation", "<f4"), ("cfo_hz", "<f4"), ("fading_index", "<f4"), ("snr_db", "<f4"), ("reserved", "<i4", 2)])
    STREAM_RESULT = np.dtype([("n_events", "<i4"), ("closed", "<i4"), ("mode", "<i4"), ("search_legs", "<i4"), ("invocations", "<u4"),
                              ("waits", "<u4"), ("rms_skips", "<u4"), ("detector_runs", "<u4"), ("rejects", "<u4"), ("near_misses", "<u4"),
                              ("weak_accepts", "<u4"), ("replays", "<u4"), ("catchups_moderate", "<u4"), ("catchups_severe", "<u4"),
                              ("reserved", "<u4", 2)])

    def stream_frame_row(self, mode):
        """bytes of one payload row of rx_stream: the window call's minimum for the mode"""
        m = capi.SEARCH_MODE[mode] if isinstance(mode, str) else int(mode)
        return max(self.window_frame_row(), 20) if m == capi.SEARCH_MODE["OFDM_LTS"] else self.MCWIN_FRAME_ROW

    def rx_stream(self, captures, capture_len, mode, control_engine=None, state=None, feed_step=0, max_invocations=1 << 20, max_events=256,
                  connected=False, carriers=10, modulation="DBPSK", spreading=1):
        """Recordings in, frames out in one call (ria_gpu_rx_stream_batch): StreamingDecoder's receive loop - search, the
        window call of the mode, the state update - for one capture per row of `captures` (float32 [n, stride] on the
        device), with state, windows, events and payloads on the device throughout.  Arguments as search(); control_engine:
        rx_window's, for "OFDM_LTS" only; state: SEARCH_STATE records (default: fresh decoders with the whole recording
        arrived for feed_step 0, nothing arrived otherwise).  A stream records at most max_events events per call; a second
        call with the returned state goes on where the first stopped.  Returns (state (SEARCH_STATE), results
        (STREAM_RESULT), events (STREAM_EVENT [n, max_events]), frames: uint8 [n, max_events, stream_frame_row(mode)] on the
        device); acquire.stream_events turns the last three into rx_stream's list form."""
        n, stride = captures.shape
        assert captures.dtype == torch.float32 and captures.is_contiguous()
        m = capi.SEARCH_MODE[mode] if isinstance(mode, str) else int(mode)
        lens = np.empty(n, np.int32)
        lens[:] = capture_len
        if state is None:
            state = self.search_state(n, fed=0 if feed_step else lens)
        st = np.ascontiguousarray(state, self.SEARCH_STATE)
        assert st.shape == (n,)
        row, ne = self.stream_frame_row(m), int(max_events)
        lens_d = torch.from_numpy(lens).to(self.device)
        st_d = torch.from_numpy(st.view(np.uint8).reshape(n, 32).copy()).to(self.device)
        res_d = torch.empty((n, 64), dtype=torch.uint8, device=self.device)
        ev_d = torch.empty((n * max(ne, 0), 64), dtype=torch.uint8, device=self.device)
        frames = torch.empty((n, max(ne, 0), row), dtype=torch.uint8, device=self.device)
        cfg = None
        if m != capi.SEARCH_MODE["OFDM_LTS"]:
            bps = {"DBPSK": 1, "DQPSK": 2}[modulation] if isinstance(modulation, str) else int(modulation)
            cfg = C.byref(capi.McdpskConfig(carriers, bps, spreading, 0))
        self._check(self.lib.ria_gpu_rx_stream_batch(self.h, control_engine.h if control_engine is not None else None, m,
                                                     capi.SEARCH_CONNECTED if connected else 0, cfg, _ptr(captures), stride, _ptr(lens_d), n,
                                                     _ptr(st_d), int(feed_step), int(max_invocations), ne, _ptr(ev_d), _ptr(frames), row,
                                                     _ptr(res_d), _stream_ptr()))
        return (self._status_array(st_d, self.SEARCH_STATE), self._status_array(res_d, self.STREAM_RESULT),
                self._status_array(ev_d, self.STREAM_EVENT).reshape(n, ne), frames)

    def rx_stream_host(self, recording, mode, control_engine=None, state=None, feed_step=0, max_invocations=1 << 20, max_events=256,
                       connected=False, carriers=10, modulation="DBPSK", spreading=1):
        """rx_stream for one recording in host memory (ria_gpu_rx_stream_host; a float32 numpy array).  Returns (state,
        results, events, frames) as rx_stream does for n = 1, frames as a numpy array."""
        x = np.ascontiguousarray(recording, np.float32)
        assert x.ndim == 1
        m = capi.SEARCH_MODE[mode] if isinstance(mode, str) else int(mode)
        if state is None:
            state = self.search_state(1, fed=0 if feed_step else len(x))
        st = np.ascontiguousarray(state, self.SEARCH_STATE).copy()
        assert st.shape == (1,)
        row, ne = self.stream_frame_row(m), int(max_events)
        ev = np.zeros(max(ne, 0), self.STREAM_EVENT)
        frames = np.zeros((1, max(ne, 0), row), np.uint8)
        res = np.zeros(1, self.STREAM_RESULT)
        cfg = None
        if m != capi.SEARCH_MODE["OFDM_LTS"]:
            bps = {"DBPSK": 1, "DQPSK": 2}[modulation] if isinstance(modulation, str) else int(modulation)
            cfg = C.byref(capi.McdpskConfig(carriers, bps, spreading, 0))
        self._check(self.lib.ria_gpu_rx_stream_host(self.h, control_engine.h if control_engine is not None else None, m,
                                                    capi.SEARCH_CONNECTED if connected else 0, cfg, x.ctypes.data, len(x), st.ctypes.data,
                                                    int(feed_step), int(max_invocations), ne, ev.ctypes.data, frames.ctypes.data, row,
                                                    res.ctypes.data))
        return st, res, ev.reshape(1, ne), frames

    MCSTREAM_STATE = np.dtype(SEARCH_STATE.descr + [("pending_total_cw", "<i4"), ("need_samples", "<i4"), ("pend_search_start", "<i4"),
                                                    ("pend_sync_position", "<i4"), ("pend_known_cfo_hz", "<f4"), ("pend_detect_threshold", "<f4"),
                                                    ("pend_min_confidence", "<f4"), ("pend_correlation", "<f4")])

    @classmethod
    def mcdpsk_stream_state(cls, n, fed=0):
        """n fresh decoder states (MCSTREAM_STATE): search_state()'s fields, then the eight pending fields, zero (searching)"""
        s = np.zeros(n, cls.MCSTREAM_STATE)
        for f in cls.SEARCH_STATE.names:
            s[f] = cls.search_state(n, fed)[f]
        return s

    def _mcstream_in(self, mode, channel_interleave, interleaver_bits, carriers, modulation, spreading):
        m = capi.SEARCH_MODE[mode] if isinstance(mode, str) else int(mode)
        bps = {"DBPSK": 1, "DQPSK": 2}[modulation] if isinstance(modulation, str) else int(modulation)
        bits = (carriers * bps if interleaver_bits is None else int(interleaver_bits)) if channel_interleave else 0
        return m, capi.McdpskConfig(carriers, bps, spreading, 0), capi.MACQ_CHANNEL_INTERLEAVE if channel_interleave else 0, bits

    def mcdpsk_stream(self, captures, capture_len, mode, state=None, feed_step=0, max_invocations=1 << 20, max_events=256, connected=False,
                      carriers=10, modulation="DBPSK", spreading=1, chase=None, cache_id=None, t0_ms=None, channel_interleave=False,
                      interleaver_bits=None):
        """rx_stream for the two MC-DPSK modes with a chase pool, channel interleaving and re-entry of a window that waits for
        samples (ria_gpu_mcdpsk_stream_batch).  state: MCSTREAM_STATE records (mcdpsk_stream_state(); default as rx_stream);
        a stream whose state comes back with pending_total_cw > 0 waits at a found sync: call again with that state and a
        longer capture.  chase: a ChasePool; stream s uses cache cache_id[s] (default s, -1 = off) and decodes a window at
        t0_ms[s] + sync_position * 1000 // 48000.  channel_interleave / interleaver_bits as in mcdpsk_window.  Returns (state
        (MCSTREAM_STATE), results (STREAM_RESULT), events (STREAM_EVENT [n, max_events]), frames uint8 [n, max_events, 320] on
        the device, harq (HARQ_RESULT [n, max_events]))."""
        n, stride = captures.shape
        assert captures.dtype == torch.float32 and captures.is_contiguous()
        m, cfg, wflags, bits = self._mcstream_in(mode, channel_interleave, interleaver_bits, carriers, modulation, spreading)
        lens = np.empty(n, np.int32)
        lens[:] = capture_len
        if state is None:
            state = self.mcdpsk_stream_state(n, fed=0 if feed_step else lens)
        st = np.ascontiguousarray(state, self.MCSTREAM_STATE)
        assert st.shape == (n,)
        row, ne = self.MCWIN_FRAME_ROW, int(max_events)
        lens_d = torch.from_numpy(lens).to(self.device)
        st_d = torch.from_numpy(st.view(np.uint8).reshape(n, 64).copy()).to(self.device)
        res_d = torch.empty((n, 64), dtype=torch.uint8, device=self.device)
        ev_d = torch.empty((n * max(ne, 0), 64), dtype=torch.uint8, device=self.device)
        harq_d = torch.empty((n * max(ne, 0), 32), dtype=torch.uint8, device=self.device)
        frames = torch.empty((n, max(ne, 0), row), dtype=torch.uint8, device=self.device)
        ids, t0, _ = self._harq_in(n, cache_id, t0_ms)
        self._check(self.lib.ria_gpu_mcdpsk_stream_batch(self.h, m, capi.SEARCH_CONNECTED if connected else 0, wflags, bits, C.byref(cfg),
                                                         _ptr(captures), stride, _ptr(lens_d), n, _ptr(st_d), int(feed_step), int(max_invocations), ne,
                                                         chase.p if chase is not None else None, _ptr(ids), _ptr(t0), _ptr(ev_d), _ptr(frames), row,
                                                         _ptr(harq_d), _ptr(res_d), _stream_ptr()))
        return (self._status_array(st_d, self.MCSTREAM_STATE), self._status_array(res_d, self.STREAM_RESULT),
                self._status_array(ev_d, self.STREAM_EVENT).reshape(n, ne), frames, self._status_array(harq_d, self.HARQ_RESULT).reshape(n, ne))

    def mcdpsk_stream_host(self, recording, mode, state=None, feed_step=0, max_invocations=1 << 20, max_events=256, connected=False,
                           carriers=10, modulation="DBPSK", spreading=1, chase=None, cache_id=0, t0_ms=0, channel_interleave=False,
                           interleaver_bits=None):
        """mcdpsk_stream for one recording in host memory (ria_gpu_mcdpsk_stream_host; a float32 numpy array).  Returns (state,
        results, events, frames, harq) as mcdpsk_stream does for n = 1, frames as a numpy array."""
        x = np.ascontiguousarray(recording, np.float32)
        assert x.ndim == 1
        m, cfg, wflags, bits = self._mcstream_in(mode, channel_interleave, interleaver_bits, carriers, modulation, spreading)
        if state is None:
            state = self.mcdpsk_stream_state(1, fed=0 if feed_step else len(x))
        st = np.ascontiguousarray(state, self.MCSTREAM_STATE).copy()
        assert st.shape == (1,)
        row, ne = self.MCWIN_FRAME_ROW, int(max_events)
        ev = np.zeros(max(ne, 0), self.STREAM_EVENT)
        harq = np.zeros(max(ne, 0), self.HARQ_RESULT)
        frames = np.zeros((1, max(ne, 0), row), np.uint8)
        res = np.zeros(1, self.STREAM_RESULT)
        self._check(self.lib.ria_gpu_mcdpsk_stream_host(self.h, m, capi.SEARCH_CONNECTED if connected else 0, wflags, bits, C.byref(cfg),
                                                        x.ctypes.data, len(x), st.ctypes.data, int(feed_step), int(max_invocations), ne,
                                                        chase.p if chase is not None else None, int(cache_id), int(t0_ms) & (2 ** 64 - 1),
                                                        ev.ctypes.data, frames.ctypes.data, row, harq.ctypes.data, res.ctypes.data))
        return st, res, ev.reshape(1, ne), frames, harq.reshape(1, ne)

    RING_STREAM_RESULT = np.dtype(STREAM_RESULT.descr + [("overflow_dropped", "<u8"), ("overflows", "<u4"), ("drift_snaps", "<u4"),
                                                         ("cursor_inits", "<u4"), ("reserved1", "<u4")])

    def rx_ring(self, captures, capture_len, mode, control_engine=None, state=None, feed_step=4800, max_invocations=1 << 20, max_events=256,
                connected=False, carriers=10, modulation="DBPSK", spreading=1):
        """rx_stream for recordings of any length (ria_gpu_rx_ring_batch): the loop on search_ring, with windows cut from the
        capture by absolute index.  state: RING_STATE records (default: fresh decoders, nothing arrived for feed_step > 0).
        The events' sync_position, search_start and next_pos are capture (absolute) indices, so acquire.stream_events and
        stream_tally work on them.  Returns (state (RING_STATE), results (RING_STREAM_RESULT), events (STREAM_EVENT
        [n, max_events]), frames: uint8 [n, max_events, stream_frame_row(mode)] on the device)."""
        n, stride = captures.shape
        assert captures.dtype == torch.float32 and captures.is_contiguous()
        m = capi.SEARCH_MODE[mode] if isinstance(mode, str) else int(mode)
        lens = np.empty(n, np.int32)
        lens[:] = capture_len
        if state is None:
            state = self.ring_state(n, total_fed=0 if feed_step else lens)
        st = np.ascontiguousarray(state, self.RING_STATE)
        assert st.shape == (n,)
        row, ne = self.stream_frame_row(m), int(max_events)
        lens_d = torch.from_numpy(lens).to(self.device)
        st_d = torch.from_numpy(st.view(np.uint8).reshape(n, 48).copy()).to(self.device)
        res_d = torch.full((n, 88), 0xAB, dtype=torch.uint8, device=self.device)
        ev_d = torch.full((n * max(ne, 0), 64), 0xAB, dtype=torch.uint8, device=self.device)
        frames = torch.full((n, max(ne, 0), row), 0xAB, dtype=torch.uint8, device=self.device)
        cfg = None
        if m != capi.SEARCH_MODE["OFDM_LTS"]:
            bps = {"DBPSK": 1, "DQPSK": 2}[modulation] if isinstance(modulation, str) else int(modulation)
            cfg = C.byref(capi.McdpskConfig(carriers, bps, spreading, 0))
        self._check(self.lib.ria_gpu_rx_ring_batch(self.h, control_engine.h if control_engine is not None else None, m,
                                                   capi.SEARCH_CONNECTED if connected else 0, cfg, _ptr(captures), stride, _ptr(lens_d), n,
                                                   _ptr(st_d), int(feed_step), int(max_invocations), ne, _ptr(ev_d), _ptr(frames), row,
                                                   _ptr(res_d), _stream_ptr()))
        return (self._status_array(st_d, self.RING_STATE), self._status_array(res_d, self.RING_STREAM_RESULT),
                self._status_array(ev_d, self.STREAM_EVENT).reshape(n, ne), frames)

    def rx_ring_host(self, recording, mode, control_engine=None, state=None, feed_step=4800, max_invocations=1 << 20, max_events=256,
                     connected=False, carriers=10, modulation="DBPSK", spreading=1):
        """rx_ring for one recording in host memory (ria_gpu_rx_ring_host; a float32 numpy array of any length in the domain).
        Returns (state, results, events, frames) as rx_ring does for n = 1, frames as a numpy array."""
        x = np.ascontiguousarray(recording, np.float32)
        assert x.ndim == 1
        m = capi.SEARCH_MODE[mode] if isinstance(mode, str) else int(mode)
        if state is None:
            state = self.ring_state(1, total_fed=0 if feed_step else len(x))
        st = np.ascontiguousarray(state, self.RING_STATE).copy()
        assert st.shape == (1,)
        row, ne = self.stream_frame_row(m), int(max_events)
        ev = np.zeros(max(ne, 0), self.STREAM_EVENT)
        frames = np.zeros((1, max(ne, 0), row), np.uint8)
        res = np.zeros(1, self.RING_STREAM_RESULT)
        cfg = None
        if m != capi.SEARCH_MODE["OFDM_LTS"]:
            bps = {"DBPSK": 1, "DQPSK": 2}[modulation] if isinstance(modulation, str) else int(modulation)
            cfg = C.byref(capi.McdpskConfig(carriers, bps, spreading, 0))
        self._check(self.lib.ria_gpu_rx_ring_host(self.h, control_engine.h if control_engine is not None else None, m,
                                                  capi.SEARCH_CONNECTED if connected else 0, cfg, x.ctypes.data, len(x), st.ctypes.data,
                                                  int(feed_step), int(max_invocations), ne, ev.ctypes.data, frames.ctypes.data, row,
                                                  res.ctypes.data))
        return st, res, ev.reshape(1, ne), frames

    MCRING_STATE = np.dtype(RING_STATE.descr + [("pending_total_cw", "<i4"), ("need_samples", "<i4"), ("pend_search_start", "<i4"),
                                                ("pend_sync_position", "<i4"), ("pend_known_cfo_hz", "<f4"), ("pend_detect_threshold", "<f4"),
                                                ("pend_min_confidence", "<f4"), ("pend_correlation", "<f4")])

    @classmethod
    def mcdpsk_ring_state(cls, n, total_fed=0):
        """n fresh decoder states (MCRING_STATE, 80 bytes): ring_state()'s fields, then the eight pending fields, zero (searching)"""
        s = np.zeros(n, cls.MCRING_STATE)
        for f in cls.RING_STATE.names:
            s[f] = cls.ring_state(n, total_fed)[f]
        return s

    def mcdpsk_ring(self, captures, capture_len, mode, state=None, feed_step=4800, max_invocations=1 << 20, max_events=256, connected=False,
                    carriers=10, modulation="DBPSK", spreading=1, chase=None, cache_id=None, t0_ms=None, channel_interleave=False,
                    interleaver_bits=None):
        """mcdpsk_stream for recordings of any length (ria_gpu_mcdpsk_ring_batch): rx_ring's loop for the two MC-DPSK modes
        with a chase pool on the audio clock (t0_ms[s] + absolute sync position * 1000 // 48000), channel interleaving and
        re-entry of a window that waits for samples.  state: MCRING_STATE records (mcdpsk_ring_state(); default: fresh
        decoders, nothing arrived for feed_step > 0); the pending positions and the events' positions are capture (absolute)
        indices.  Returns (state (MCRING_STATE), results (RING_STREAM_RESULT), events (STREAM_EVENT [n, max_events]), frames
        uint8 [n, max_events, 320] on the device, harq (HARQ_RESULT [n, max_events]))."""
        n, stride = captures.shape
        assert captures.dtype == torch.float32 and captures.is_contiguous()
        m, cfg, wflags, bits = self._mcstream_in(mode, channel_interleave, interleaver_bits, carriers, modulation, spreading)
        lens = np.empty(n, np.int32)
        lens[:] = capture_len
        if state is None:
            state = self.mcdpsk_ring_state(n, total_fed=0 if feed_step else lens)
        st = np.ascontiguousarray(state, self.MCRING_STATE)
        assert st.shape == (n,)
        row, ne = self.MCWIN_FRAME_ROW, int(max_events)
        lens_d = torch.from_numpy(lens).to(self.device)
        st_d = torch.from_numpy(st.view(np.uint8).reshape(n, 80).copy()).to(self.device)
        res_d = torch.empty((n, 88), dtype=torch.uint8, device=self.device)
        ev_d = torch.empty((n * max(ne, 0), 64), dtype=torch.uint8, device=self.device)
        harq_d = torch.empty((n * max(ne, 0), 32), dtype=torch.uint8, device=self.device)
        frames = torch.empty((n, max(ne, 0), row), dtype=torch.uint8, device=self.device)
        ids, t0, _ = self._harq_in(n, cache_id, t0_ms)
        self._check(self.lib.ria_gpu_mcdpsk_ring_batch(self.h, m, capi.SEARCH_CONNECTED if connected else 0, wflags, bits, C.byref(cfg),
                                                       _ptr(captures), stride, _ptr(lens_d), n, _ptr(st_d), int(feed_step), int(max_invocations), ne,
                                                       chase.p if chase is not None else None, _ptr(ids), _ptr(t0), _ptr(ev_d), _ptr(frames), row,
                                                       _ptr(harq_d), _ptr(res_d), _stream_ptr()))
        return (self._status_array(st_d, self.MCRING_STATE), self._status_array(res_d, self.RING_STREAM_RESULT),
                self._status_array(ev_d, self.STREAM_EVENT).reshape(n, ne), frames, self._status_array(harq_d, self.HARQ_RESULT).reshape(n, ne))

    def mcdpsk_ring_host(self, recording, mode, state=None, feed_step=4800, max_invocations=1 << 20, max_events=256, connected=False,
                         carriers=10, modulation="DBPSK", spreading=1, chase=None, cache_id=0, t0_ms=0, channel_interleave=False,
                         interleaver_bits=None):
        """mcdpsk_ring for one recording in host memory (ria_gpu_mcdpsk_ring_host; a float32 numpy array of any length in the
        domain).  Returns (state, results, events, frames, harq) as mcdpsk_ring does for n = 1, frames as a numpy array."""
        x = np.ascontiguousarray(recording, np.float32)
        assert x.ndim == 1
        m, cfg, wflags, bits = self._mcstream_in(mode, channel_interleave, interleaver_bits, carriers, modulation, spreading)
        if state is None:
            state = self.mcdpsk_ring_state(1, total_fed=0 if feed_step else len(x))
        st = np.ascontiguousarray(state, self.MCRING_STATE).copy()
        assert st.shape == (1,)
        row, ne = self.MCWIN_FRAME_ROW, int(max_events)
        ev = np.zeros(max(ne, 0), self.STREAM_EVENT)
        harq = np.zeros(max(ne, 0), self.HARQ_RESULT)
        frames = np.zeros((1, max(ne, 0), row), np.uint8)
        res = np.zeros(1, self.RING_STREAM_RESULT)
        self._check(self.lib.ria_gpu_mcdpsk_ring_host(self.h, m, capi.SEARCH_CONNECTED if connected else 0, wflags, bits, C.byref(cfg),
                                                      x.ctypes.data, len(x), st.ctypes.data, int(feed_step), int(max_invocations), ne,
                                                      chase.p if chase is not None else None, int(cache_id), int(t0_ms) & (2 ** 64 - 1),
                                                      ev.ctypes.data, frames.ctypes.data, row, harq.ctypes.data, res.ctypes.data))
        return st, res, ev.reshape(1, ne), frames, harq.reshape(1, ne)

    MCDFRAME_RESULT =np.dtype([("success", "u1"), ("codewords_ok", "u1"), ("codewords_failed", "u1"), ("frame_type", "u1"),
                                ("header_total_cw", "<i4"), ("frame_bytes", "<i4"), ("reserved", "<i4")])
    HARQ_RESULT = np.dtype([("seq", "<u2"), ("valid", "u1"), ("entry", "u1"), ("src_hash", "<u4"), ("dst_hash", "<u4"),
                            ("stored_mask", "<u2"), ("sum_mask", "<u2"), ("recovered_mask", "<u2"), ("max_combine", "u1"),
                            ("reserved0", "u1"), ("cache_id", "<i4"), ("reserved", "<i4", 2)])

    def chase_pool(self, n_caches, max_entries=16, ttl_ms=30000):
        return ChasePool(self, n_caches, max_entries, ttl_ms)

    def _harq_in(self, n, cache_id, now_ms):
        ids = np.arange(n, dtype=np.int32) if cache_id is None else np.ascontiguousarray(np.broadcast_to(np.asarray(cache_id, np.int32), (n,)))
        now = np.ascontiguousarray(np.broadcast_to(np.asarray(0 if now_ms is None else now_ms, np.uint64), (n,)))
        return (torch.from_numpy(ids.copy()).to(self.device), torch.from_numpy(now.view(np.int64).copy()).to(self.device),
                torch.empty((n, 32), dtype=torch.uint8, device=self.device))

    def mcdpsk_decode_frame(self, llr, n_llr=None, chase=None, cache_id=None, now_ms=None, channel_interleave=False, interleaver_bits=None,
                            carriers=10, modulation="DBPSK"):
        """StreamingDecoder::decodeMCDPSKFrame at R1/4 over rows of soft bits (ria_gpu_mcdpsk_decode_frame_batch): llr float32
        [n, 648 .. 16 * 648], n_llr the soft bits of each row (None: the whole row).  chase: a ChasePool; row f then uses cache
        cache_id[f] (default f, -1 = off) at time now_ms (scalar or per row, default 0).
        channel_interleave: decodeMCDPSKFrame with use_mc_dpsk_channel_interleave_ (ria_gpu_mcdpsk_decode_frame_ci_batch);
        interleaver_bits None: carriers x bits of `modulation`.  The result then has the fields cw0_deinterleaved and ci_tried.
        Returns (frame bytes uint8 [n, 20 * (cols // 648)], result (MCDFRAME_RESULT), harq result (HARQ_RESULT))."""
        n, stride = llr.shape
        assert llr.dtype == torch.float32 and llr.is_contiguous()
        row = 20 * (stride // 648)
        frames = torch.empty((n, row), dtype=torch.uint8, device=self.device)
        res = torch.empty((n, 16), dtype=torch.uint8, device=self.device)
        nl = None
        if n_llr is not None:
            nl = torch.as_tensor(np.ascontiguousarray(n_llr, np.int32)).to(self.device) if not torch.is_tensor(n_llr) else n_llr
            assert nl.dtype == torch.int32 and nl.numel() == n and nl.is_contiguous()
        ids, now, harq = self._harq_in(n, cache_id, now_ms)
        if channel_interleave:
            bps = {"DBPSK": 1, "DQPSK": 2}[modulation] if isinstance(modulation, str) else int(modulation)
            bits = carriers * bps if interleaver_bits is None else int(interleaver_bits)
            self._check(self.lib.ria_gpu_mcdpsk_decode_frame_ci_batch(self.h, _ptr(llr), stride, _ptr(nl), n, chase.p if chase is not None else None,
                                                                      _ptr(ids), _ptr(now), _ptr(frames), row, _ptr(res), _ptr(harq),
                                                                      capi.MACQ_CHANNEL_INTERLEAVE, bits, _stream_ptr()))
            r = self._status_array(res, self.MCDFRAME_RESULT)
            return frames, self._ci_fields(r, r["reserved"]), self._status_array(harq, self.HARQ_RESULT)
        self._check(self.lib.ria_gpu_mcdpsk_decode_frame_batch(self.h, _ptr(llr), stride, _ptr(nl), n, chase.p if chase is not None else None,
                                                               _ptr(ids), _ptr(now), _ptr(frames), row, _ptr(res), _ptr(harq), _stream_ptr()))
        return frames, self._status_array(res, self.MCDFRAME_RESULT), self._status_array(harq, self.HARQ_RESULT)

    def mcdpsk_modulate(self, data, carriers=10, bits_per_symbol=1, spreading=1):
        data = np.ascontiguousarray(data, np.uint8)
        cfg = capi.McdpskConfig(carriers, bits_per_symbol, spreading, 0)
        out = np.zeros(600000, np.float32)
        n = self.lib.ria_gpu_mcdpsk_modulate_host(self.h, C.byref(cfg), data.ctypes.data, len(data), out.ctypes.data, len(out))
        if n < 0:
            raise capi.RiaError("mcdpsk_modulate failed")
        return out[:n].copy()

    def mcdpsk_interleave(self, coded, interleaver_bits):
        """ChannelInterleaver(interleaver_bits, 648)::interleave over codewords of 81 coded bytes
        (ria_gpu_mcdpsk_interleave_batch): coded uint8 [..., 81 * k] (device tensor or host array) -> a new tensor of that shape"""
        if not torch.is_tensor(coded):
            coded = torch.from_numpy(np.ascontiguousarray(coded, np.uint8)).to(self.device)
        assert coded.dtype == torch.uint8 and coded.is_contiguous() and coded.shape[-1] % 81 == 0
        out = torch.empty_like(coded)
        self._check(self.lib.ria_gpu_mcdpsk_interleave_batch(self.h, int(interleaver_bits), _ptr(coded), coded.numel() // 81, _ptr(out), _stream_ptr()))
        return out

    def mcdpsk_modulate_batch(self, data, carriers=10, bits_per_symbol=1, spreading=1):
        """MultiCarrierDPSKModulator on the device: data uint8 [n, n_bytes] (device tensor or host array) -> float32 [n, samples]"""
        if not torch.is_tensor(data):
            data = torch.from_numpy(np.ascontiguousarray(data, np.uint8)).to(self.device)
        assert data.dtype == torch.uint8 and data.is_contiguous() and data.dim() == 2
        n, nb = data.shape
        bits = carriers * bits_per_symbol
        fs = (9 + ((nb * 8 + bits - 1) // bits) * spreading) * 512
        out = torch.empty((n, fs), dtype=torch.float32, device=self.device)
        cfg = capi.McdpskConfig(carriers, bits_per_symbol, spreading, 0)
        self._check(self.lib.ria_gpu_mcdpsk_modulate_batch(self.h, C.byref(cfg), _ptr(data), nb, n, _ptr(out), fs, _stream_ptr()))
        return out

    def chase_combine(self, acc, count, soft, decoded=None):
        """ChaseCache::store arithmetic in place on acc [n,648] / count [n] (int32); returns stored flags."""
        n = acc.shape[0]
        stored = torch.zeros(n, dtype=torch.uint8, device=self.device)
        self._check(self.lib.ria_gpu_chase_combine_batch(self.h, _ptr(acc), _ptr(count), _ptr(decoded), _ptr(soft), n,
                                                         _ptr(stored), _stream_ptr()))
        return stored

    def channel_exact_(self, samples, kind, snr_db, seed, first_frame=0):
        """Reference-identical channel (mt19937 stream, seed + first_frame + f per frame); in place, any frame length."""
        n, fs = samples.shape
        assert samples.dtype == torch.float32 and samples.is_contiguous()
        self._check(self.lib.ria_gpu_channel_exact_batch(self.h, int(kind), float(snr_db), int(seed) & 0xffffffff, int(first_frame),
                                                         _ptr(samples), fs, fs, n, _stream_ptr()))
        return samples

    def channel_exact_seeded_(self, samples, kind, snr_db, seeds):
        """Reference-identical channel with one mt19937 seed per frame: seeds uint32 tensor/array [n]; in place."""
        n, fs = samples.shape
        assert samples.dtype == torch.float32 and samples.is_contiguous()
        if not torch.is_tensor(seeds):
            seeds = torch.from_numpy(np.ascontiguousarray(seeds, np.uint32).view(np.int32)).to(self.device)
        assert seeds.numel() == n and seeds.element_size() == 4 and seeds.is_contiguous()
        self._check(self.lib.ria_gpu_channel_exact_seeded_batch(self.h, int(kind), float(snr_db), _ptr(seeds), _ptr(samples), fs, fs, n,
                                                                _stream_ptr()))
        return samples

    def channel_exact_cfo_(self, samples, kind, snr_db, seeds, cfo_hz=None, random_cfo_max_hz=0.0):
        """Reference-identical channel incl. its CFO impairment (Config::cfo_hz per frame / random_cfo_max_hz + applyCFO);
        in place.  Returns the per-frame getActualCFO() tensor."""
        n, fs = samples.shape
        assert samples.dtype == torch.float32 and samples.is_contiguous()
        if not torch.is_tensor(seeds):
            seeds = torch.from_numpy(np.ascontiguousarray(seeds, np.uint32).view(np.int32)).to(self.device)
        assert seeds.numel() == n and seeds.element_size() == 4 and seeds.is_contiguous()
        if cfo_hz is not None and not torch.is_tensor(cfo_hz):
            cfo_hz = torch.from_numpy(np.full(n, cfo_hz, np.float32) if np.ndim(cfo_hz) == 0 else np.ascontiguousarray(cfo_hz, np.float32)).to(self.device)
        assert cfo_hz is None or (cfo_hz.dtype == torch.float32 and cfo_hz.numel() == n and cfo_hz.is_contiguous())
        actual = torch.zeros(n, dtype=torch.float32, device=self.device)
        self._check(self.lib.ria_gpu_channel_exact_cfo_batch(self.h, int(kind), float(snr_db), _ptr(seeds), _ptr(cfo_hz), float(random_cfo_max_hz),
                                                             _ptr(actual), _ptr(samples), fs, fs, n, _stream_ptr()))
        return actual

    def tx_cfo(self, samples, cfo_hz, phase=None):
        """SimulatedChannel::applyTxCFO over a batch: samples float32 [n, len] on the device, cfo_hz scalar or [n];
        phase float32 [n] accumulator (updated in place) or None.  Returns the shifted samples."""
        n, L = samples.shape
        assert samples.dtype == torch.float32 and samples.is_contiguous()
        if not torch.is_tensor(cfo_hz):
            cfo_hz = torch.from_numpy(np.full(n, cfo_hz, np.float32) if np.ndim(cfo_hz) == 0 else np.ascontiguousarray(cfo_hz, np.float32)).to(self.device)
        assert cfo_hz.dtype == torch.float32 and cfo_hz.numel() == n and cfo_hz.is_contiguous()
        assert phase is None or (phase.dtype == torch.float32 and phase.numel() == n and phase.is_contiguous())
        out = torch.empty_like(samples)
        self._check(self.lib.ria_gpu_tx_cfo_batch(self.h, _ptr(samples), L, L, n, _ptr(cfo_hz), _ptr(phase), _ptr(out), L, _stream_ptr()))
        return out

    def burst_deinterleave(self, llr, burst_frames):
        """BurstInterleaver::deinterleave: llr float32 [n_groups*N, >=2592] physical -> logical (same shape)."""
        n, stride = llr.shape
        assert llr.dtype == torch.float32 and llr.is_contiguous() and n % burst_frames == 0
        out = torch.zeros_like(llr)
        self._check(self.lib.ria_gpu_burst_deinterleave_batch(self.h, _ptr(llr), stride, burst_frames, n // burst_frames, _ptr(out), _stream_ptr()))
        return out

    def burst_interleave(self, coded, burst_frames):
        """BurstInterleaver::interleave: coded uint8 [n_groups*N, 324] logical -> physical."""
        n = coded.shape[0]
        assert coded.dtype == torch.uint8 and coded.is_contiguous() and coded.shape[1] == 324 and n % burst_frames == 0
        out = torch.zeros_like(coded)
        self._check(self.lib.ria_gpu_burst_interleave_batch(self.h, _ptr(coded), burst_frames, n // burst_frames, _ptr(out), _stream_ptr()))
        return out

    def debug_math(self, op, a, b=None):
        out = torch.empty_like(a)
        self._check(self.lib.ria_gpu_debug_math(self.h, op, _ptr(a), _ptr(b), a.numel(), _ptr(out), _stream_ptr()))
        return out

    def frame_status(self, st):
        return self._status_array(st, self.FRAME_STATUS)

    def decode_status(self, st):
        return self._status_array(st, self.DECODE_STATUS)
