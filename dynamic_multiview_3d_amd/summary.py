"""TensorFlow event files with scalar summaries, written without TensorFlow -- the counterpart of the reference's
tf.summary.FileWriter + log_value (mv3d/utils/tf_utils.py:11-15; mv3d/nobg_dm.py:143-145 logs `test_loss` through it), so the
numbers land where TensorBoard looks for them.

An event file is a TFRecord file (read_tf_records.py: length, masked CRC-32C of the length, payload, masked CRC-32C of the
payload) of serialized `Event` messages:
    Event   { double wall_time = 1; int64 step = 2; string file_version = 3; Summary summary = 5; }
    Summary { repeated Value value = 1; }      Value { string tag = 1; float simple_value = 2; }
The first record is Event{wall_time, file_version: "brain.Event:2"}.  Fields holding their default (step 0) are left out, as a
proto3 serializer does.  Scalars only: image and histogram summaries are not written.
"""
import os
import socket
import struct
import time

from .read_tf_records import TFRecordWriter, read_records, _fields, _enc_varint, _ld

FILE_VERSION = b'brain.Event:2'


def encode_event(wall_time, step=0, file_version=None, scalars=()):
    """Serialized Event; scalars: (tag, value) pairs that become one Summary."""
    out = b'\x09' + struct.pack('<d', float(wall_time))                         # field 1, 64-bit
    if int(step) != 0:
        out += b'\x10' + _enc_varint(int(step) & 0xFFFFFFFFFFFFFFFF)            # field 2, varint (two's complement int64)
    if file_version is not None:
        out += _ld(3, bytes(file_version))
    if scalars:
        summary = b''
        for tag, value in scalars:
            summary += _ld(1, _ld(1, tag.encode('utf-8')) + b'\x15' + struct.pack('<f', float(value)))     # Value: tag, simple_value
        out += _ld(5, summary)
    return out


def decode_event(data):
    """{'wall_time', 'step', 'file_version' (or None), 'scalars': [(tag, value), ...]} of one serialized Event."""
    ev = {'wall_time': 0.0, 'step': 0, 'file_version': None, 'scalars': []}
    for num, wt, v in _fields(memoryview(data)):
        if num == 1 and wt == 1:
            ev['wall_time'] = struct.unpack('<d', bytes(v))[0]
        elif num == 2 and wt == 0:
            ev['step'] = v - (1 << 64) if v >= (1 << 63) else v
        elif num == 3 and wt == 2:
            ev['file_version'] = bytes(v).decode('utf-8')
        elif num == 5 and wt == 2:
            for snum, swt, value in _fields(v):
                if snum != 1 or swt != 2:
                    continue
                tag, simple = None, None
                for vnum, vwt, vv in _fields(value):
                    if vnum == 1 and vwt == 2:
                        tag = bytes(vv).decode('utf-8')
                    elif vnum == 2 and vwt == 5:
                        simple = struct.unpack('<f', bytes(vv))[0]
                if tag is not None and simple is not None:
                    ev['scalars'].append((tag, simple))
    return ev


def read_events(path):
    """Every event of one file, record checksums verified (IOError on a corrupted or truncated file)."""
    return [decode_event(data) for data in read_records(path, verify=True)]


class FileWriter:
    """tf.summary.FileWriter(logdir): creates `logdir/events.out.tfevents.<secs>.<hostname>` and writes the version event.
    clock: the source of wall_time (time.time; a test passes a fixed one)."""

    def __init__(self, logdir, clock=time.time, hostname=None):
        self.clock = clock
        os.makedirs(logdir, exist_ok=True)
        now = clock()
        self.path = os.path.join(logdir, 'events.out.tfevents.%010d.%s' % (int(now), hostname or socket.gethostname()))
        self._w = TFRecordWriter(self.path)
        self.add_event(encode_event(now, file_version=FILE_VERSION))
        self.flush()

    def add_event(self, event):
        """event: a serialized Event (encode_event)."""
        if self._w is None:
            raise ValueError("FileWriter is closed")
        self._w.write(event)

    def add_scalar(self, tag, value, step):
        self.add_event(encode_event(self.clock(), step=step, scalars=[(tag, value)]))

    def flush(self):
        if self._w is not None:
            self._w.f.flush()

    def close(self):
        if self._w is not None:
            self._w.close()
            self._w = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def log_value(writer, value, tag, step):
    """mv3d/utils/tf_utils.py:11-15: one Event{wall_time, step, summary{value{tag, simple_value}}}."""
    writer.add_scalar(tag, value, step)
