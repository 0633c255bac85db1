"""The host's part of ria_amd.acquire.rx_stream (acquire.py:553-594), one statement per function, in the numpy types that
loop uses: what ria_amd/csrc/stream_rules.hpp must compute.  tests/test_stream_rules_host.py compares the two case by case;
tests/test_gpu_stream_call.py uses comparator(), the same loop with its state returned."""
import numpy as np

from ria_amd import capi

OFDM, MCDPSK = 0, 1
NONE = -2 ** 31
CLOSED = capi.STREAM_CLOSED


def _names(family):
    return {v: k for k, v in (capi.WIN_OUTCOME if family == OFDM else capi.MWIN_OUTCOME).items()}


def window_len(full, capture_len, search_start):
    return int(min(full, capture_len - search_start))                                   # :555


def min_confidence(conf, corr):
    return np.minimum(np.float32(conf), np.float32(corr))                               # :559


def rebase_last_sync(last, search_start):
    last_in = np.array([last], np.int32).astype(np.int64)                               # :567-568
    return int(np.where(last_in == capi.SEARCH_NO_LAST_SYNC, capi.MWIN_NO_LAST_SYNC,
                        np.clip(last_in - search_start, -2 ** 31 + 1, 2 ** 31 - 1))[0])


def moved(family, outcome):
    if family == OFDM:                                                                  # :564
        return outcome == capi.WIN_OUTCOME["DECODED"] or outcome == capi.WIN_OUTCOME["CONTROL_PROFILE"]
    return outcome == capi.MWIN_OUTCOME["DECODED"]                                      # :574


def last_sync(family, delivered, sync_position, state_last, window_last, search_start):
    state = np.zeros(1, np.int32)
    if family == OFDM:
        state[0] = np.where(delivered, np.int32(sync_position), np.int32(state_last))   # :565, :585
    else:
        out_last = np.array([window_last], np.int32).astype(np.int64)                   # :575-576
        state[0] = np.where(out_last == capi.MWIN_NO_LAST_SYNC, capi.SEARCH_NO_LAST_SYNC, out_last + np.int32(search_start))[0].astype(np.int32)
    return int(state[0])


def cursor(family, outcome, next_pos, search_start, sync_position, first_frame, cursor_in):
    if next_pos >= 0:                                                                   # :586-589
        return int(search_start) + int(next_pos)
    if _names(family).get(outcome) in ("BURST", "TOO_LONG"):
        return int(sync_position) + first_frame
    return cursor_in


def fed(fed_in, capture_len, cursor_now):
    return max(int(fed_in), min(int(capture_len), int(cursor_now)))                     # :592


def close(family, outcome, n_events, max_events, cursor_now):
    """0 = the stream stays open (:593); else the reason, in the order ria_gpu_rx_stream_batch reports it"""
    if _names(family).get(outcome) == "NEED_SAMPLES":
        return CLOSED["WINDOW_NEED_SAMPLES"]
    if n_events >= max_events:
        return CLOSED["EVENTS_FULL"]
    if cursor_now >= capi.SEARCH_MAX_CAPTURE:
        return CLOSED["RING_END"]
    return 0


def comparator(engine, captures, capture_len, mode, control_engine=None, state=None, feed_step=0, max_invocations=1 << 20, max_events=256,
               connected=False, carriers=10, modulation="DBPSK", spreading=1):
    """ria_amd.acquire.rx_stream statement for statement (its lines are cited), with the state given and returned and the
    reason every stream closed for: (events, state, closed).  test_gpu_stream_call.py asserts that its events equal
    rx_stream's own before it is used as the reference for the state."""
    import torch
    from ria_amd.acquire import _gather_windows, mcdpsk_frame_len
    n = captures.shape[0]
    m = capi.SEARCH_MODE[mode] if isinstance(mode, str) else int(mode)
    ofdm = m == capi.SEARCH_MODE["OFDM_LTS"]
    chirp = m == capi.SEARCH_MODE["MCDPSK_CHIRP"]
    lens = np.empty(n, np.int64)
    lens[:] = capture_len
    state = engine.search_state(n, fed=0 if feed_step else lens) if state is None else np.array(state, engine.SEARCH_STATE)
    bps = {"DBPSK": 1, "DQPSK": 2}[modulation] if isinstance(modulation, str) else int(modulation)
    search_len = capi.SEARCH_MIN_SEARCH[m]
    first_frame = engine.geo.frame_samples if ofdm else mcdpsk_frame_len(1, carriers, bps, spreading)
    full = search_len + (engine.geo.frame_samples + 32 if ofdm else mcdpsk_frame_len(8, carriers, bps, spreading))
    names = _names(OFDM if ofdm else MCDPSK)
    events = [[] for _ in range(n)]
    closed = np.zeros(n, np.int64)
    open_ = np.ones(n, bool)
    while open_.any():
        idx = np.flatnonzero(open_)
        res, st = engine.search(captures[torch.as_tensor(idx, device=captures.device)].contiguous() if len(idx) < n else captures, lens[idx],
                                state[idx], m, feed_step=feed_step, max_invocations=max_invocations, connected=connected, carriers=carriers,
                                modulation=modulation, spreading=spreading)
        state[idx] = st
        found = res["outcome"] == capi.SEARCH_OUTCOME["SYNC_FOUND"]
        open_[idx[~found]] = False
        closed[idx[~found]] = res["outcome"][~found]
        by_len = {}
        for j in np.flatnonzero(found):
            by_len.setdefault(int(min(full, lens[idx[j]] - res["search_start"][j])), []).append(j)
        for wl, js in by_len.items():
            rows, r = idx[js], res[js]
            w = _gather_windows(captures, rows, r["search_start"], wl)
            conf = np.minimum(r["min_confidence"], r["correlation"])
            if ofdm:
                frames, wres, acq, _, _ = engine.rx_window(control_engine, w, search_len, known_cfo=r["known_cfo_hz"], detect_threshold=r["detect_threshold"],
                                                           min_confidence=conf, abs_base=r["search_start"])
                nbytes, ok, fading = wres["frame"]["frame_bytes"], (wres["frame"]["success"] != 0) | (wres["frame"]["codewords_ok"] != 0), wres["fading_index"]
                cfo, mv = wres["sync_cfo_hz"], (wres["outcome"] == capi.WIN_OUTCOME["DECODED"]) | (wres["outcome"] == capi.WIN_OUTCOME["CONTROL_PROFILE"])
                last = np.where(ok, r["sync_position"], state["last_decoded_sync_pos"][rows])
            else:
                last_in = state["last_decoded_sync_pos"][rows].astype(np.int64)
                rel = np.where(last_in == capi.SEARCH_NO_LAST_SYNC, capi.MWIN_NO_LAST_SYNC, np.clip(last_in - r["search_start"], -2 ** 31 + 1, 2 ** 31 - 1))
                frames, wres, acq, _ = engine.mcdpsk_window(w, search_len, carriers=carriers, modulation=bps, spreading=spreading,
                                                            sync="chirp" if chirp else "zc", disconnected=chirp and not connected,
                                                            known_cfo=r["known_cfo_hz"], detect_threshold=r["detect_threshold"], min_confidence=conf,
                                                            abs_base=r["search_start"], last_decoded_sync=rel)
                nbytes, ok, fading = acq["frame_bytes"], wres["deliver"] != 0, acq["fading_index"]
                cfo, mv = acq["cfo_hz"], wres["outcome"] == capi.MWIN_OUTCOME["DECODED"]
                out_last = wres["last_decoded_sync"].astype(np.int64)
                last = np.where(out_last == capi.MWIN_NO_LAST_SYNC, capi.SEARCH_NO_LAST_SYNC, out_last + r["search_start"])
            frames = frames.cpu().numpy()
            for k, s in enumerate(rows):
                name = names[int(wres["outcome"][k])]
                events[s].append(dict(position=int(r["sync_position"][k]), outcome=name,
                                      frame=frames[k, :int(nbytes[k])].tobytes() if ok[k] else None))
                if mv[k]:
                    state["last_cfo_hz"][s] = cfo[k]
                    state["fading_hint"][s] = fading[k]
                state["last_decoded_sync_pos"][s] = last[k]
                if wres["next_pos"][k] >= 0:
                    state["correlation_pos"][s] = int(r["search_start"][k]) + int(wres["next_pos"][k])
                elif name in ("BURST", "TOO_LONG"):
                    state["correlation_pos"][s] = int(r["sync_position"][k]) + first_frame
                state["fed"][s] = max(int(state["fed"][s]), min(int(lens[s]), int(state["correlation_pos"][s])))
                if name == "NEED_SAMPLES" or len(events[s]) >= max_events or state["correlation_pos"][s] >= capi.SEARCH_MAX_CAPTURE:
                    open_[s] = False
                    closed[s] = close(OFDM if ofdm else MCDPSK, int(wres["outcome"][k]), len(events[s]), max_events, int(state["correlation_pos"][s]))
    return events, state, closed
