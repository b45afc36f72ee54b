"""The voice consumer restated in plain Python (TEST INFRASTRUCTURE ONLY): the rules of include/m17hip.h (m17hip_voice_fetch, ABI 606) over the
frame records of ONE channel, record by record, state carried between feeds — the yardstick the device consumer (csrc/m17_voice_kernel.hpp) is held
against.  The oracle supplies the records (oracle_lib.demod); this supplies the planes and the calls they must become.  Slow and obvious on purpose:
one record at a time, no numpy in the rules."""
import numpy as np

FT_LSF, FT_STREAM = 0, 2
MARK_BLANK, MARK_EOS, MARK_FIRST, MARK_GAP = 1, 2, 4, 8
CLOSE_EOS, CLOSE_LSF = 1, 2

CALL_REC = np.dtype([("channel", "<u4"), ("seq", "<u4"), ("start_pos", "<u8"), ("end_pos", "<u8"), ("cost_sum", "<u4"), ("frames", "<u4"),
                     ("blanked", "<u4"), ("lost", "<u4"), ("has_lsf", "u1"), ("close", "u1"), ("lsf", "u1", (30,))])
assert CALL_REC.itemsize == 72


class VoiceLog:
    """One channel.  feed(records) -> (audio [n][16] uint8, marks [n] uint8, calls closed by these records as a CALL_REC array); `call` is the
    open call (a dict) or None, `seq` the calls closed since the reset."""

    def __init__(self, channel=0):
        self.channel = channel
        self.reset()

    def reset(self):
        self.call, self.seq = None, 0

    def _open(self, pos, lsf):
        self.call = dict(start_pos=pos, end_pos=pos, cost_sum=0, frames=0, blanked=0, lost=0, has_lsf=0 if lsf is None else 1,
                         lsf=bytes(30) if lsf is None else bytes(lsf), prev_fn=None)

    def _close(self, how, out):
        c = self.call
        out.append((self.channel, self.seq, c["start_pos"], c["end_pos"], c["cost_sum"], c["frames"], c["blanked"], c["lost"], c["has_lsf"], how,
                    np.frombuffer(c["lsf"], dtype=np.uint8)))
        self.seq += 1
        self.call = None

    def feed(self, records):
        audio, marks, closed = [], [], []
        for r in records:
            ftype, pos, cost = int(r["frame_type"]), int(r["sample_pos"]), int(r["cost"])
            payload = bytes(r["payload"])
            if ftype == FT_LSF:                                   # rule 1
                if self.call is not None:
                    self._close(CLOSE_LSF, closed)
                self._open(pos, payload[:30])
                continue
            if ftype != FT_STREAM:                                # rule 3
                continue
            if self.call is None:                                 # rule 2
                self._open(pos, None)
            c = self.call
            fn = ((payload[0] << 8) | payload[1]) & 0x7FFF
            mark = 0
            if cost > 80:
                mark |= MARK_BLANK
            if cost < 70 and payload[0] & 0x80:
                mark |= MARK_EOS
            if c["frames"] == 0:
                mark |= MARK_FIRST
            elif fn != (c["prev_fn"] + 1) % 0x8000:
                mark |= MARK_GAP
                c["lost"] = (c["lost"] + (fn - c["prev_fn"] - 1) % 0x8000) & 0xFFFFFFFF
            audio.append(payload[2:18])
            marks.append(mark)
            c["frames"] += 1
            c["blanked"] += mark & MARK_BLANK
            c["cost_sum"] = (c["cost_sum"] + cost) & 0xFFFFFFFF
            c["end_pos"] = pos
            c["prev_fn"] = fn
            if mark & MARK_EOS:
                self._close(CLOSE_EOS, closed)
        a = np.frombuffer(b"".join(audio), dtype=np.uint8).reshape(-1, 16) if audio else np.zeros((0, 16), dtype=np.uint8)
        calls = np.zeros(len(closed), dtype=CALL_REC)
        for i, row in enumerate(closed):
            calls[i] = row
        return a, np.array(marks, dtype=np.uint8), calls


class VoiceBank:
    """`channels` VoiceLogs side by side: feed(rows) with rows[c] the records of channel c -> (audio [C][n][16], marks [C][n], counts [C], calls in
    (channel, seq) order), n = the largest count (at least `slots` when given), rows zero-padded."""

    def __init__(self, channels, channel_base=0):
        self.logs = [VoiceLog(channel_base + c) for c in range(channels)]

    def feed(self, rows, slots=None):
        parts = [log.feed(r) for log, r in zip(self.logs, rows)]
        counts = np.array([p[1].size for p in parts], dtype=np.uint32)
        n = max(int(counts.max()) if counts.size else 0, slots or 0)
        audio = np.zeros((len(parts), n, 16), dtype=np.uint8)
        marks = np.zeros((len(parts), n), dtype=np.uint8)
        for c, (a, m, _) in enumerate(parts):
            audio[c, :m.size], marks[c, :m.size] = a, m
        calls = np.concatenate([p[2] for p in parts]) if parts else np.zeros(0, dtype=CALL_REC)
        return audio, marks, counts, calls
