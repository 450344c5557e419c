"""ternary-image-codec_amd — host-side Python mirror of the reference's Word27 API over libt3hip.so (HIP, gfx950).

The names follow the reference (old/include/ternary_image_codec_v6_min.hpp = OLD): ProfileID, UEPLayout helpers,
EncoderContext / DecoderContext, encode_raw_pixels_to_words, decode_raw_words_to_pixels, encode_profile_from_raw,
decode_profile_to_raw (+ encode_frame / decode_frame conveniences).  Arrays are numpy: pixels as the structured
dtype PIXEL_DT (u16 Yq, i16 Cbq, i16 Crq = PixelYCbCrQuant OLD:670-674), words as uint8 [n, 9] (Word27 OLD:666-669).

This module is plumbing over the C-ABI in include/t3hip.h.  There is NO CPU fallback: if the HIP library is missing
or no gfx950 device is usable, compute calls raise T3Error.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("T3HIP_LIB", os.path.join(_HERE, "libt3hip.so"))   # T3HIP_LIB: timing-only ablation builds

PIXEL_DT = np.dtype([("Yq", "<u2"), ("Cbq", "<i2"), ("Crq", "<i2")])

OK, E_NODEVICE, E_HIP, E_ARG, E_CAPACITY, E_HEADER, E_RS, E_COMM = 0, -1, -2, -3, -4, -5, -6, -7
MODE_COMPAT, MODE_FIXED = 0, 1


class ProfileID:  # OLD:34
    RAW_MODE = 0xFF
    P1_RS26_24 = 0
    P2_RS26_22 = 1
    P3_RS26_20 = 2
    P4_RS26_18 = 3
    P5_RS26_22_2D = 4


class Cfg(C.Structure):
    """t3_cfg: POD mirror of EncoderConfig (OLD:862-873) / DecoderConfigSeen (OLD:874-884) + mode."""
    _fields_ = [("profile", C.c_uint8), ("band_profile", C.c_uint8 * 9), ("tile_w", C.c_uint16), ("tile_h", C.c_uint16),
                ("seed_a", C.c_uint32), ("seed_b", C.c_uint32), ("seed_s0", C.c_uint32),
                ("beacon_words_period", C.c_uint32), ("beacon_band_slot", C.c_uint8), ("beacon_enabled", C.c_uint8),
                ("subword", C.c_uint8), ("centered", C.c_uint8), ("superframe_words", C.c_uint32),
                ("coset", C.c_uint8), ("mode", C.c_uint8), ("reserved", C.c_uint8 * 2)]

    def as_dict(self):
        return dict(profile=self.profile, band_profile=list(self.band_profile), tile_w=self.tile_w, tile_h=self.tile_h,
                    seed_a=self.seed_a, seed_b=self.seed_b, seed_s0=self.seed_s0,
                    beacon_words_period=self.beacon_words_period, beacon_band_slot=self.beacon_band_slot,
                    beacon_enabled=self.beacon_enabled, subword=self.subword, centered=self.centered,
                    superframe_words=self.superframe_words, coset=self.coset, mode=self.mode)

    def copy(self):
        c = Cfg()
        C.memmove(C.byref(c), C.byref(self), C.sizeof(Cfg))
        return c


class Layout(C.Structure):
    _fields_ = [("n_raw_words", C.c_uint64), ("n_sym", C.c_uint64), ("band_len", C.c_uint64 * 9), ("band_blocks", C.c_uint64 * 9),
                ("band_body_off", C.c_uint64 * 9), ("body_syms", C.c_uint64), ("body_syms_framed", C.c_uint64),
                ("out_syms", C.c_uint64), ("out_words", C.c_uint64), ("header_syms", C.c_uint32), ("band_k", C.c_uint8 * 9),
                ("interleave2d", C.c_uint8), ("beacon_on", C.c_uint8), ("pad_", C.c_uint8)]


class FrameRecord(C.Structure):
    _fields_ = [("frame_idx", C.c_uint64), ("n_words", C.c_uint64), ("byte_offset", C.c_uint64), ("crc32", C.c_uint32),
                ("sym_sum", C.c_uint32), ("header_syms", C.c_uint8 * 54), ("profile", C.c_uint8), ("mode", C.c_uint8), ("pad_", C.c_uint8 * 8)]


FRAME_RECORD_BYTES = C.sizeof(FrameRecord)


class T3Error(RuntimeError):
    """code: the T3_E_* value.  needed: on E_CAPACITY from an entry point that reports it, the size the output must have (in the units of
    its capacity argument: words, pixels, bytes, trits or symbols); None otherwise."""

    def __init__(self, code, where="", needed=None):
        self.code = code
        self.needed = needed if code == E_CAPACITY else None
        msg = "%s: %s" % (where, strerror(code))
        if code == E_HIP:
            msg += " [" + last_hip_error() + "]"
        if code == E_COMM:
            msg += " [" + lib().t3hip_comm_last_error().decode() + "]"
        super().__init__(msg)


_lib_handle = None


def lib():
    """The C-ABI library; raises loudly when it has not been built (no fallback path exists)."""
    global _lib_handle
    if _lib_handle is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("HIP extension missing: %s (run `python -c 'import __graft_entry__ as g; g.build()'`)" % LIB_PATH)
        try:
            # One HIP runtime per process: PyTorch-ROCm bundles its own libamdhip64.so.7; when torch is going to be
            # used next to this library (tests, bench.py) it must be the first to load it, and libt3hip.so then binds
            # to that already-loaded runtime by SONAME.  Without torch the system runtime under /opt/rocm is used.
            import torch  # noqa: F401
        except Exception:
            pass
        L = C.CDLL(LIB_PATH)
        L.t3hip_strerror.restype = C.c_char_p
        L.t3hip_last_hip_error.restype = C.c_char_p
        L.t3hip_version.restype = C.c_char_p
        L.t3hip_comm_last_error.restype = C.c_char_p
        L.t3hip_encoded_words.restype = C.c_uint64
        L.t3hip_frame_record_scratch_bytes.restype = C.c_uint64
        _lib_handle = L
    return _lib_handle


def strerror(code):
    return lib().t3hip_strerror(C.c_int(code)).decode()


def last_hip_error():
    return lib().t3hip_last_hip_error().decode()


def version():
    return lib().t3hip_version().decode()


def device_count():
    return lib().t3hip_device_count()


def init(device=0):
    rc = lib().t3hip_init(C.c_int(device))
    if rc != OK:
        raise T3Error(rc, "t3hip_init(%d)" % device)


def is_ready():
    return bool(lib().t3hip_is_ready())


class Context:
    """One GPU's context (t3hip_create): own stream, tables and scratch.  `use()` binds the CALLING THREAD to it -- every call of this
    module made by that thread then runs on it -- `use_default()` goes back to the process default (init())."""

    def __init__(self, device=0):
        self.h = C.c_void_p()
        _chk(lib().t3hip_create(C.c_int(device), C.byref(self.h)), "t3hip_create(%d)" % device)

    def use(self):
        _chk(lib().t3hip_use(self.h), "t3hip_use")

    @staticmethod
    def use_default():
        _chk(lib().t3hip_use(C.c_void_p()), "t3hip_use(NULL)")

    def device(self):
        return lib().t3hip_ctx_device(self.h)

    def destroy(self):
        if self.h:
            _chk(lib().t3hip_destroy(self.h), "t3hip_destroy"); self.h = C.c_void_p()


def _chk(rc, where, n_out=None):
    """n_out: the call's size output (a ctypes integer); what it holds goes into T3Error.needed when the call refused for capacity."""
    if rc != OK:
        raise T3Error(rc, where, None if n_out is None else int(n_out.value))


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- config helpers (reference names) ----------------------------------------------------------------
def default_cfg():
    c = Cfg()
    lib().t3hip_cfg_default(C.byref(c))
    return c


def uep_uniform(cfg, idx=1):  # OLD:64-67
    for i in range(9):
        cfg.band_profile[i] = idx % 4


def uep_luma_priority(cfg):  # OLD:68-72
    for i in range(9):
        cfg.band_profile[i] = 1
    cfg.band_profile[0] = cfg.band_profile[3] = cfg.band_profile[6] = 2


def make_cfg(profile=ProfileID.P2_RS26_22, uep=1, tile=(0, 0), seed=(1, 1, 1), beacon=(0, 0, 0), superframe_words=8192,
             subword=27, centered=1, coset=0, mode=MODE_COMPAT):
    c = default_cfg()
    c.profile = profile
    if uep == "luma":
        uep_luma_priority(c)
    elif isinstance(uep, int):
        uep_uniform(c, uep)
    else:
        for i in range(9):
            c.band_profile[i] = uep[i]
    c.tile_w, c.tile_h = tile
    c.seed_a, c.seed_b, c.seed_s0 = seed
    c.beacon_words_period, c.beacon_band_slot, c.beacon_enabled = beacon
    c.superframe_words, c.subword, c.centered, c.coset, c.mode = superframe_words, subword, centered, coset, mode
    return c


class EncoderContext:  # OLD:885-900
    def __init__(self, mode=MODE_COMPAT):
        self.cfg = default_cfg()
        self.cfg.mode = mode


class DecoderContext:  # OLD:901-916
    def __init__(self, mode=MODE_COMPAT):
        self.cfg_last_seen = default_cfg()
        self.cfg_last_seen.mode = mode


# ---- host-only metadata ----------------------------------------------------------------------------------
def plan(n_raw_words, cfg):
    L = Layout()
    _chk(lib().t3hip_plan(C.c_uint64(n_raw_words), C.byref(cfg), C.byref(L)), "t3hip_plan")
    return L


def encoded_words(n_raw_words, cfg):
    return lib().t3hip_encoded_words(C.c_uint64(n_raw_words), C.byref(cfg))


def gf27_tables():
    e = np.zeros(78, np.uint8); lg = np.zeros(27, np.int16); m = np.zeros(729, np.uint8); iv = np.zeros(27, np.uint8)
    _chk(lib().t3hip_gf27_tables(_vp(e), _vp(lg), _vp(m), _vp(iv)), "t3hip_gf27_tables")
    return dict(exp=e, log=lg, mul=m, inv=iv)


def rs_generator(k):
    g = np.zeros(27 - k, np.uint8)
    _chk(lib().t3hip_rs_generator(C.c_int(k), _vp(g)), "t3hip_rs_generator")
    return g


def rs_parity_matrix(k, mode=MODE_COMPAT):
    P = np.zeros((k, 26 - k), np.uint8)
    _chk(lib().t3hip_rs_parity_matrix(C.c_int(k), C.c_int(mode), _vp(P)), "t3hip_rs_parity_matrix")
    return P


def header_pack(cfg, frame_seq=0, band_map_hash=0):
    s = np.zeros(27, np.uint8)
    _chk(lib().t3hip_header_pack(C.byref(cfg), C.c_uint32(frame_seq), C.c_uint32(band_map_hash), _vp(s)), "t3hip_header_pack")
    return s


def header_check(syms):
    s = np.ascontiguousarray(syms, np.uint8)
    return bool(lib().t3hip_header_check(_vp(s)))


def header_unpack(syms):
    s = np.ascontiguousarray(syms, np.uint8); c = default_cfg(); fs = C.c_uint32(); bh = C.c_uint32()
    _chk(lib().t3hip_header_unpack(_vp(s), C.byref(c), C.byref(fs), C.byref(bh)), "t3hip_header_unpack")
    return c, fs.value, bh.value


def header_encode(cfg, n_raw_words):
    out = np.zeros(96, np.uint8); n = C.c_uint32()
    _chk(lib().t3hip_header_encode(C.byref(cfg), C.c_uint64(n_raw_words), _vp(out), C.byref(n)), "t3hip_header_encode")
    return out[: n.value].copy()


# ---- host-buffer API (the reference's std::vector functions) ------------------------------------------------
def encode_raw_pixels_to_words(px):  # OLD:723-734
    px = np.ascontiguousarray(px, PIXEL_DT)
    out = np.zeros(((len(px) + 1) // 2, 9), np.uint8)
    _chk(lib().t3hip_pack_pixels(_vp(px), C.c_uint64(len(px)), _vp(out)), "t3hip_pack_pixels")
    return out


def decode_raw_words_to_pixels(words):  # OLD:735-747
    words = np.ascontiguousarray(words, np.uint8).reshape(-1, 9)
    px = np.zeros(2 * len(words), PIXEL_DT)
    _chk(lib().t3hip_unpack_words(_vp(words), C.c_uint64(len(words)), _vp(px)), "t3hip_unpack_words")
    return px


_VALID_SUB = (27, 24, 21, 18, 15)


def encode_raw_pixels_to_words_subword(px, sub):  # NEWH:119-121 / NEWC:139-146: validates `sub`, else identical
    if sub not in _VALID_SUB:
        return None
    return encode_raw_pixels_to_words(px)


def decode_raw_words_to_pixels_subword(words, sub):  # NEWH:123-125 / NEWC:148-155
    if sub not in _VALID_SUB:
        return None
    return decode_raw_words_to_pixels(words)


# ---- subword trit streams and wire packings (OLD:834-859, TPACK:18-65) ----------------------------
def _u8(a):
    return np.ascontiguousarray(a, np.uint8).reshape(-1)


def extract_subword_stream_from_words(words, N):  # OLD:834-844 -> uint8 trits, N per word
    w = np.ascontiguousarray(words, np.uint8).reshape(-1, 9); n = len(w)
    out = np.zeros(n * int(N), np.uint8)
    _chk(lib().t3hip_subword_extract(_vp(w), C.c_uint64(n), C.c_int(int(N)), _vp(out)), "t3hip_subword_extract")
    return out


def build_words_from_subword_stream(trits, N, fill=0):  # OLD:845-859 -> Word27 array
    t = _u8(trits)
    lib().t3hip_subword_words.restype = C.c_uint64
    cap = int(lib().t3hip_subword_words(C.c_uint64(len(t)), C.c_int(int(N))))
    out = np.zeros((cap, 9), np.uint8); nw = C.c_uint64()
    _chk(lib().t3hip_subword_build(_vp(t), C.c_uint64(len(t)), C.c_int(int(N)), C.c_uint8(fill), _vp(out), C.c_uint64(cap), C.byref(nw)), "t3hip_subword_build", nw)
    return out[: nw.value]


def ut_to_base243(trits):  # TPACK:28-38
    t = _u8(trits)
    lib().t3hip_base243_bytes.restype = C.c_uint64
    cap = int(lib().t3hip_base243_bytes(C.c_uint64(len(t))))
    out = np.zeros(cap, np.uint8); nb = C.c_uint64()
    _chk(lib().t3hip_base243_pack(_vp(t), C.c_uint64(len(t)), _vp(out), C.c_uint64(cap), C.byref(nb)), "t3hip_base243_pack", nb)
    return out[: nb.value]


def base243_to_ut(data):  # TPACK:40-50 -> trits, or None where the reference returns false
    b = _u8(data)
    cap = 5 * max(len(b), 4)
    out = np.zeros(cap, np.uint8); nt = C.c_uint64()
    rc = lib().t3hip_base243_unpack(_vp(b), C.c_uint64(len(b)), _vp(out), C.c_uint64(cap), C.byref(nt))
    if rc == E_HEADER:
        return None
    _chk(rc, "t3hip_base243_unpack", nt)
    return out[: nt.value]


def blit_center_rgb(src, sw, sh, cw, ch):  # io_image.hpp:125-140 -> uint8 canvas (ch, cw, 3)
    a = _u8(src)
    if len(a) != sw * sh * 3:
        raise ValueError("blit_center_rgb: %d bytes for a %dx%d image" % (len(a), sw, sh))
    out = np.zeros(cw * ch * 3, np.uint8)
    _chk(lib().t3hip_blit_center_rgb(_vp(a), C.c_int(sw), C.c_int(sh), _vp(out), C.c_int(cw), C.c_int(ch)), "t3hip_blit_center_rgb")
    return out.reshape(ch, cw, 3)


def extract_center_q(full, fw, fh, sw, sh):  # io_image.hpp:215-235 -> pixel records (sh * sw)
    f = np.ascontiguousarray(full)
    raw = f.view(np.uint8).reshape(-1)
    if len(raw) != fw * fh * 6:
        raise ValueError("extract_center_q: %d bytes for a %dx%d frame" % (len(raw), fw, fh))
    out = np.zeros(sw * sh * 6, np.uint8)
    _chk(lib().t3hip_extract_center_q(_vp(raw), C.c_int(fw), C.c_int(fh), _vp(out), C.c_int(sw), C.c_int(sh)), "t3hip_extract_center_q")
    return out.view(f.dtype) if f.dtype.itemsize == 6 else out


def blit_center_rgb_dev(d_src, sw, sh, d_dst, cw, ch, stream=0):
    _chk(lib().t3hip_blit_center_rgb_dev(C.c_void_p(d_src), C.c_int(sw), C.c_int(sh), C.c_void_p(d_dst), C.c_int(cw), C.c_int(ch), C.c_void_p(stream)), "t3hip_blit_center_rgb_dev")


def extract_center_q_dev(d_full, fw, fh, d_sub, sw, sh, stream=0):
    _chk(lib().t3hip_extract_center_q_dev(C.c_void_p(d_full), C.c_int(fw), C.c_int(fh), C.c_void_p(d_sub), C.c_int(sw), C.c_int(sh), C.c_void_p(stream)), "t3hip_extract_center_q_dev")


def words_to_bytes(words):  # TPACK:53-58
    w = np.ascontiguousarray(words, np.uint8).reshape(-1)
    out = np.zeros(len(w), np.uint8)
    _chk(lib().t3hip_mod27_bytes(_vp(w), C.c_uint64(len(w)), _vp(out)), "t3hip_mod27_bytes")
    return out


def bytes_to_words(data):  # TPACK:60-65: nothing unless len % 9 == 0
    b = _u8(data)
    if len(b) % 9:
        return np.zeros((0, 9), np.uint8)
    out = np.zeros(len(b), np.uint8)
    _chk(lib().t3hip_mod27_bytes(_vp(b), C.c_uint64(len(b)), _vp(out)), "t3hip_mod27_bytes")
    return out.reshape(-1, 9)


# ---- RGB8 <-> quantised YCbCr bridge (old/include/io_image.hpp:156-195) ---------------------------------
def rgb_to_quant_stream(rgb):  # (n, 3) or flat uint8 RGB -> PixelYCbCrQuant array
    r = _u8(rgb); n = len(r) // 3
    px = np.zeros(n, PIXEL_DT)
    _chk(lib().t3hip_rgb_to_quant(_vp(r), C.c_uint64(n), _vp(px)), "t3hip_rgb_to_quant")
    return px


def quant_stream_to_rgb(px):  # PixelYCbCrQuant array -> flat uint8 RGB
    p = np.ascontiguousarray(px, PIXEL_DT)
    out = np.zeros(3 * len(p), np.uint8)
    _chk(lib().t3hip_quant_to_rgb(_vp(p), C.c_uint64(len(p)), _vp(out)), "t3hip_quant_to_rgb")
    return out


def rgb_to_quant_dev(d_rgb, n_px, d_px, stream=0):
    _chk(lib().t3hip_rgb_to_quant_dev(C.c_void_p(d_rgb), C.c_uint64(n_px), C.c_void_p(d_px), C.c_void_p(stream)), "t3hip_rgb_to_quant_dev")


def quant_to_rgb_dev(d_px, n_px, d_rgb, stream=0):
    _chk(lib().t3hip_quant_to_rgb_dev(C.c_void_p(d_px), C.c_uint64(n_px), C.c_void_p(d_rgb), C.c_void_p(stream)), "t3hip_quant_to_rgb_dev")


def encode_rgb_dev(d_rgb, n_px, cfg, d_out, cap_words, stream=0):
    """RGB8 frame (device) -> coded stream: bridge kernel + fused encode on `stream`; returns the coded word count."""
    n = C.c_uint64()
    _chk(lib().t3hip_encode_rgb_dev(C.c_void_p(d_rgb), C.c_uint64(n_px), C.byref(cfg), C.c_void_p(d_out), C.c_uint64(cap_words), C.byref(n), C.c_void_p(stream)), "t3hip_encode_rgb_dev", n)
    return n.value


def decode_rgb_async(d_in, n_in, cfg, n_px, d_rgb, d_verdict, stream=0):
    """Coded stream -> RGB8 frame with the stream's known configuration (streaming decode entry + bridge kernel)."""
    _chk(lib().t3hip_decode_rgb_async(C.c_void_p(d_in), C.c_uint64(n_in), C.byref(cfg), C.c_uint64(n_px), C.c_void_p(d_rgb), C.c_void_p(d_verdict), C.c_void_p(stream)), "t3hip_decode_rgb_async")


# ---- window decode and the image front end (old/include/io_image.hpp:102-140, 237-337; include/t3hip.h) --------------------
class WindowPlan(C.Structure):
    """t3_window_plan: the tiles a window decode launches and the run of stream pixels they produce."""
    _fields_ = [("n_tiles", C.c_uint32), ("tile_lo", C.c_uint32), ("tile_hi", C.c_uint32), ("first_px", C.c_uint64), ("n_px", C.c_uint64),
                ("tile_range", C.c_uint8), ("pad_", C.c_uint8 * 7)]


WINDOW_PIXELS, WINDOW_RGB = 1, 2


def window_plan(n_raw_words, cfg, fw, fh, x0, y0, w, h):  # host only
    p = WindowPlan()
    _chk(lib().t3hip_window_plan(C.c_uint64(n_raw_words), C.byref(cfg), C.c_uint32(fw), C.c_uint32(fh), C.c_uint32(x0), C.c_uint32(y0),
                                 C.c_uint32(w), C.c_uint32(h), C.byref(p)), "t3hip_window_plan")
    return p


def decode_window_async(d_in, n_in, cfg, n_raw, fw, fh, x0, y0, w, h, d_out, out_fmt, d_verdict, stream=0):
    """The w x h window at (x0, y0) of a coded frame read as rows of fw pixels; out_fmt WINDOW_PIXELS (6 B) or WINDOW_RGB (3 B)."""
    _chk(lib().t3hip_decode_window_async(C.c_void_p(d_in), C.c_uint64(n_in), C.byref(cfg), C.c_uint64(n_raw), C.c_uint32(fw), C.c_uint32(fh),
                                         C.c_uint32(x0), C.c_uint32(y0), C.c_uint32(w), C.c_uint32(h), C.c_void_p(d_out), C.c_int(out_fmt),
                                         C.c_void_p(d_verdict), C.c_void_p(stream)), "t3hip_decode_window_async")


def image_geometry(sub, centered):  # host only -> (fw, fh, x0, y0, tw, th)
    v = [C.c_int() for _ in range(6)]
    _chk(lib().t3hip_image_geometry(C.c_int(int(sub)), C.c_int(1 if centered else 0), *[C.byref(x) for x in v]), "t3hip_image_geometry")
    return tuple(x.value for x in v)


def resize_rgb_nn(src, sw, sh, dw, dh):  # io_image.hpp:102-124 -> uint8 (dh, dw, 3)
    a = _u8(src)
    if len(a) != max(sw, 0) * max(sh, 0) * 3:
        raise ValueError("resize_rgb_nn: %d bytes for a %dx%d image" % (len(a), sw, sh))
    out = np.zeros(dw * dh * 3, np.uint8)
    _chk(lib().t3hip_resize_rgb_nn(_vp(a), C.c_int(sw), C.c_int(sh), _vp(out), C.c_int(dw), C.c_int(dh)), "t3hip_resize_rgb_nn")
    return out.reshape(dh, dw, 3)


def image_compose(src, sw, sh, sub, centered):  # resize to std_res_for(sub) + centring blit -> uint8 (fh, fw, 3)
    a = _u8(src)
    if len(a) != max(sw, 0) * max(sh, 0) * 3:
        raise ValueError("image_compose: %d bytes for a %dx%d image" % (len(a), sw, sh))
    fw, fh = image_geometry(sub, centered)[:2]
    out = np.zeros(fw * fh * 3, np.uint8)
    _chk(lib().t3hip_image_compose(_vp(a), C.c_int(sw), C.c_int(sh), C.c_int(int(sub)), C.c_int(1 if centered else 0), _vp(out)), "t3hip_image_compose")
    return out.reshape(fh, fw, 3)


def resize_rgb_nn_dev(d_src, sw, sh, d_dst, dw, dh, stream=0):
    _chk(lib().t3hip_resize_rgb_nn_dev(C.c_void_p(d_src), C.c_int(sw), C.c_int(sh), C.c_void_p(d_dst), C.c_int(dw), C.c_int(dh), C.c_void_p(stream)), "t3hip_resize_rgb_nn_dev")


def image_compose_dev(d_src, sw, sh, sub, centered, d_frame_rgb, stream=0):
    _chk(lib().t3hip_image_compose_dev(C.c_void_p(d_src), C.c_int(sw), C.c_int(sh), C.c_int(int(sub)), C.c_int(1 if centered else 0), C.c_void_p(d_frame_rgb),
                                       C.c_void_p(stream)), "t3hip_image_compose_dev")


def encode_image_dev(d_src, sw, sh, sub, centered, cfg, d_out, cap_words, stream=0):
    """RGB8 image of any size (device) -> coded frame of its subword mode's geometry; returns the coded word count."""
    n = C.c_uint64()
    _chk(lib().t3hip_encode_image_dev(C.c_void_p(d_src), C.c_int(sw), C.c_int(sh), C.c_int(int(sub)), C.c_int(1 if centered else 0), C.byref(cfg),
                                      C.c_void_p(d_out), C.c_uint64(cap_words), C.byref(n), C.c_void_p(stream)), "t3hip_encode_image_dev", n)
    return n.value


def decode_image_async(d_in, n_in, cfg, sub, centered, d_rgb, d_verdict, stream=0):
    """Coded frame -> the target-sized RGB8 image (tw * th * 3 bytes) of image_geometry(sub, centered)."""
    _chk(lib().t3hip_decode_image_async(C.c_void_p(d_in), C.c_uint64(n_in), C.byref(cfg), C.c_int(int(sub)), C.c_int(1 if centered else 0),
                                        C.c_void_p(d_rgb), C.c_void_p(d_verdict), C.c_void_p(stream)), "t3hip_decode_image_async")


def subword_extract_dev(d_words, n_words, N, d_trits, stream=0):
    _chk(lib().t3hip_subword_extract_dev(C.c_void_p(d_words), C.c_uint64(n_words), C.c_int(int(N)), C.c_void_p(d_trits), C.c_void_p(stream)), "t3hip_subword_extract_dev")


def subword_build_dev(d_trits, n_trits, N, fill, d_words, cap_words, stream=0):
    nw = C.c_uint64()
    _chk(lib().t3hip_subword_build_dev(C.c_void_p(d_trits), C.c_uint64(n_trits), C.c_int(int(N)), C.c_uint8(fill), C.c_void_p(d_words), C.c_uint64(cap_words), C.byref(nw), C.c_void_p(stream)), "t3hip_subword_build_dev", nw)
    return nw.value


def base243_pack_dev(d_trits, n_trits, d_out, cap_bytes, stream=0):
    nb = C.c_uint64()
    _chk(lib().t3hip_base243_pack_dev(C.c_void_p(d_trits), C.c_uint64(n_trits), C.c_void_p(d_out), C.c_uint64(cap_bytes), C.byref(nb), C.c_void_p(stream)), "t3hip_base243_pack_dev", nb)
    return nb.value


def base243_unpack_dev(d_in, n_bytes, total, d_trits, stream=0):
    _chk(lib().t3hip_base243_unpack_dev(C.c_void_p(d_in), C.c_uint64(n_bytes), C.c_uint64(total), C.c_void_p(d_trits), C.c_void_p(stream)), "t3hip_base243_unpack_dev")


def encode_profile_from_raw(raw_words, ectx):  # OLD:1043-1169 -> (True, words)
    cfg = ectx.cfg if isinstance(ectx, EncoderContext) else ectx
    raw = np.ascontiguousarray(raw_words, np.uint8).reshape(-1, 9)
    cap = encoded_words(len(raw), cfg)
    out = np.zeros((cap, 9), np.uint8); n = C.c_uint64()
    _chk(lib().t3hip_encode_profile(_vp(raw), C.c_uint64(len(raw)), C.byref(cfg), _vp(out), C.c_uint64(cap), C.byref(n)), "t3hip_encode_profile", n)
    return True, out[: n.value]


def encode_frame(px, ectx):  # pack + profile encode in one fused launch
    cfg = ectx.cfg if isinstance(ectx, EncoderContext) else ectx
    px = np.ascontiguousarray(px, PIXEL_DT)
    cap = encoded_words((len(px) + 1) // 2, cfg)
    out = np.zeros((cap, 9), np.uint8); n = C.c_uint64()
    _chk(lib().t3hip_encode_frame(_vp(px), C.c_uint64(len(px)), C.byref(cfg), _vp(out), C.c_uint64(cap), C.byref(n)), "t3hip_encode_frame", n)
    return True, out[: n.value]


def _decode(fn, words, dctx, unit_dt, units_per_word, where):
    seen = dctx.cfg_last_seen if isinstance(dctx, DecoderContext) else dctx
    words = np.ascontiguousarray(words, np.uint8).reshape(-1, 9)
    cap = units_per_word * (len(words) + 16)
    out = np.zeros(cap if unit_dt is PIXEL_DT else (cap, 9), unit_dt); n = C.c_uint64()
    rc = fn(_vp(words), C.c_uint64(len(words)), C.byref(seen), _vp(out), C.c_uint64(cap), C.byref(n))
    if rc in (E_HEADER, E_RS):  # the reference's `false`: output left empty (OLD:997)
        return False, out[:0]
    _chk(rc, where, n)
    return True, out[: n.value]


def decode_profile_to_raw(words, dctx):  # OLD:995-1041 -> (ok, raw words); mutates dctx.cfg_last_seen like the reference
    return _decode(lib().t3hip_decode_profile, words, dctx, np.uint8, 1, "t3hip_decode_profile")


def decode_frame(words, dctx):
    return _decode(lib().t3hip_decode_frame, words, dctx, PIXEL_DT, 2, "t3hip_decode_frame")


# ---- the reference decoder's stages one at a time (OLD:918-993; decode_profile_to_raw fuses them) -------------------------------
def _codes(code_k, code_mode):
    return (C.c_uint8 * 4)(*[int(x) for x in code_k]), (C.c_uint8 * 4)(*[int(x) for x in code_mode])


def read_and_decode_header_from_words(words, cursor, mode=MODE_COMPAT, k=18):
    """Stage 1 (OLD:918-937) on the host: -> (ok, cursor, cfg, frame_seq, band_map_hash).  cursor stays put when fewer than six
    words remain, else it advances by six before decoding (also on a false); the two 26-symbol blocks are decoded with RS(26, k)
    in arithmetic `mode` (t3hip_rs_decode_block_host), the hp symbols are a18[0..17] + b18[0..8].  cfg is None on a false; a k other
    than 18 gives a false (the reference overruns its 18-symbol buffers for k > 18)."""
    w = np.ascontiguousarray(words, np.uint8).reshape(-1, 9)
    if cursor + 6 > len(w):
        return False, cursor, None, 0, 0
    sy = w[cursor: cursor + 6].reshape(-1)
    cursor += 6
    if k != 18:
        return False, cursor, None, 0, 0
    hp = np.zeros(27, np.uint8)
    for blk, (lo, n_keep) in enumerate(((0, 18), (26, 9))):
        code = np.ascontiguousarray(sy[lo: lo + 26]).copy(); data = np.zeros(18, np.uint8)
        rc = lib().t3hip_rs_decode_block_host(C.c_int(k), C.c_int(mode), _vp(code), _vp(data))
        if rc == 0:
            return False, cursor, None, 0, 0
        _chk(0 if rc == 1 else rc, "t3hip_rs_decode_block_host")
        hp[18 * blk: 18 * blk + n_keep] = data[:n_keep]
    if not header_check(hp):
        return False, cursor, None, 0, 0
    cfg, fs, bh = header_unpack(hp)
    cfg.mode = mode
    return True, cursor, cfg, fs, bh


def descramble_words(words, a, b, s0):
    """Stage 2 (OLD:938-947) on host words: uploaded, descramble_words_kernel, downloaded -> new uint8 [n, 9] array."""
    w = np.ascontiguousarray(words, np.uint8).reshape(-1, 9).copy()
    _chk(lib().t3hip_descramble_words(_vp(w), C.c_uint64(len(w)), C.c_uint32(a), C.c_uint32(b), C.c_uint32(s0)), "t3hip_descramble_words")
    return w


def descramble_words_dev(d_words, n_words, a, b, s0, stream=0):
    """In place on 9 * n_words device bytes at any alignment, asynchronous on `stream`."""
    _chk(lib().t3hip_descramble_words_dev(C.c_void_p(d_words), C.c_uint64(n_words), C.c_uint32(a), C.c_uint32(b), C.c_uint32(s0), C.c_void_p(stream)), "t3hip_descramble_words_dev")


def demap_rsdecode_bands_syms(n_words, hdr, code_k):
    """Output size of stage 3 for a body of n_words words (0 on bad arguments)."""
    lib().t3hip_demap_rsdecode_bands_syms.restype = C.c_uint64
    ks, _ = _codes(code_k, (0, 0, 0, 0))
    return int(lib().t3hip_demap_rsdecode_bands_syms(C.c_uint64(n_words), C.byref(hdr), ks))


def demap_rsdecode_bands(body, hdr, code_k, code_mode):
    """Stage 3 (OLD:948-993) on a descrambled host body -> (ok, syms).  hdr: a Cfg whose band_profile and beacon_* fields are read;
    band b uses code band_profile[b] % 4 = RS(26, code_k[q]) in arithmetic code_mode[q].  ok False: syms = the symbols of the blocks
    in front of the first one that does not decode, as the reference leaves out_syms."""
    w = np.ascontiguousarray(body, np.uint8).reshape(-1, 9)
    ks, ms = _codes(code_k, code_mode)
    cap = demap_rsdecode_bands_syms(len(w), hdr, code_k)
    out = np.zeros(cap, np.uint8); n = C.c_uint64()
    rc = lib().t3hip_demap_rsdecode_bands(_vp(w), C.c_uint64(len(w)), C.byref(hdr), ks, ms, _vp(out), C.c_uint64(cap), C.byref(n))
    if rc == E_RS:
        return False, out[: n.value]
    _chk(rc, "t3hip_demap_rsdecode_bands", n)
    return True, out[: n.value]


def demap_rsdecode_bands_dev(d_body, n_words, hdr, code_k, code_mode, d_out, cap, d_n_valid, stream=0):
    """Asynchronous on `stream`; d_n_valid (device uint64) ends as the valid prefix (= the returned size when every block decoded)."""
    ks, ms = _codes(code_k, code_mode)
    rc = lib().t3hip_demap_rsdecode_bands_dev(C.c_void_p(d_body), C.c_uint64(n_words), C.byref(hdr), ks, ms, C.c_void_p(d_out), C.c_uint64(cap),
                                              C.c_void_p(d_n_valid), C.c_void_p(stream))
    if rc != OK:   # (the entry has no size output: the plan is asked)
        raise T3Error(rc, "t3hip_demap_rsdecode_bands_dev", demap_rsdecode_bands_syms(n_words, hdr, code_k))
    return demap_rsdecode_bands_syms(n_words, hdr, code_k)


# ---- device-resident API: raw device pointers (ints) + hipStream_t (int) -----------------------------------------
def pack_pixels_dev(d_px, n_px, d_words, stream=0):
    _chk(lib().t3hip_pack_pixels_dev(C.c_void_p(d_px), C.c_uint64(n_px), C.c_void_p(d_words), C.c_void_p(stream)), "t3hip_pack_pixels_dev")


def unpack_words_dev(d_words, n_words, d_px, stream=0):
    _chk(lib().t3hip_unpack_words_dev(C.c_void_p(d_words), C.c_uint64(n_words), C.c_void_p(d_px), C.c_void_p(stream)), "t3hip_unpack_words_dev")


def encode_profile_dev(d_raw, n_raw, cfg, d_out, cap_words, stream=0):
    n = C.c_uint64()
    _chk(lib().t3hip_encode_profile_dev(C.c_void_p(d_raw), C.c_uint64(n_raw), C.byref(cfg), C.c_void_p(d_out), C.c_uint64(cap_words), C.byref(n), C.c_void_p(stream)), "t3hip_encode_profile_dev", n)
    return n.value


def encode_frame_dev(d_px, n_px, cfg, d_out, cap_words, stream=0):
    n = C.c_uint64()
    _chk(lib().t3hip_encode_frame_dev(C.c_void_p(d_px), C.c_uint64(n_px), C.byref(cfg), C.c_void_p(d_out), C.c_uint64(cap_words), C.byref(n), C.c_void_p(stream)), "t3hip_encode_frame_dev", n)
    return n.value


def decode_profile_dev(d_in, n_in, seen, d_out, cap_units, to_pixels=False, stream=0):
    """Returns (rc, n_out): rc is OK, E_HEADER or E_RS (the reference's bool); other codes raise."""
    n = C.c_uint64()
    rc = lib().t3hip_decode_profile_dev(C.c_void_p(d_in), C.c_uint64(n_in), C.byref(seen), C.c_void_p(d_out), C.c_uint64(cap_units), C.byref(n), C.c_int(1 if to_pixels else 0), C.c_void_p(stream))
    if rc not in (OK, E_HEADER, E_RS):
        raise T3Error(rc, "t3hip_decode_profile_dev", n.value)
    return rc, n.value


def read_header_dev(d_in, n_in, mode, stream=0):
    c = default_cfg(); c.mode = mode; n = C.c_uint64()
    rc = lib().t3hip_read_header_dev(C.c_void_p(d_in), C.c_uint64(n_in), C.c_int(mode), C.byref(c), C.byref(n), C.c_void_p(stream))
    if rc not in (OK, E_HEADER):
        raise T3Error(rc, "t3hip_read_header_dev")
    return rc, c, n.value


def decode_body_dev(d_in, n_in, cfg, n_raw, d_out, cap_units, d_fail, to_pixels=False, stream=0):
    n = C.c_uint64()
    _chk(lib().t3hip_decode_body_dev(C.c_void_p(d_in), C.c_uint64(n_in), C.byref(cfg), C.c_uint64(n_raw), C.c_void_p(d_out), C.c_uint64(cap_units), C.byref(n),
                                     C.c_int(1 if to_pixels else 0), C.c_void_p(d_fail), C.c_void_p(stream)), "t3hip_decode_body_dev", n)
    return n.value


def decode_frame_async(d_in, n_in, cfg, n_raw, d_out, cap_units, d_verdict, to_pixels=True, stream=0):
    """Streaming decode with a known configuration, no synchronisation; d_verdict -> two device uint32: [0] header differs,
    [1] uncorrectable blocks.  Returns the unit count the launch will produce."""
    n = C.c_uint64()
    _chk(lib().t3hip_decode_frame_async(C.c_void_p(d_in), C.c_uint64(n_in), C.byref(cfg), C.c_uint64(n_raw), C.c_void_p(d_out), C.c_uint64(cap_units), C.byref(n),
                                        C.c_int(1 if to_pixels else 0), C.c_void_p(d_verdict), C.c_void_p(stream)), "t3hip_decode_frame_async", n)
    return n.value


# ---- repair of a FIXED coded frame in place: corrected codewords on the wire, no pixels (include/t3hip.h) ---------------------
class RepairPlan(C.Structure):
    """t3_repair_plan: the kernel that serves the framing (path 1 fused, 0 generic), its tiles, the frame's coded bytes."""
    _fields_ = [("path", C.c_uint8), ("pad_", C.c_uint8 * 3), ("n_tiles", C.c_uint32), ("blocks_per_tile", C.c_uint32), ("pad2_", C.c_uint32),
                ("in_bytes", C.c_uint64)]


REPAIR_WRITE = 1                                        # without it a repair call is a dry run: the same counts, no byte stored


def repair_plan(n_raw_words, cfg):  # host only
    p = RepairPlan()
    _chk(lib().t3hip_repair_plan(C.c_uint64(n_raw_words), C.byref(cfg) if cfg is not None else None, C.byref(p)), "t3hip_repair_plan")
    return p


def repair_frame_async(d_io, n_in, cfg, n_raw, flags, d_verdict, stream=0):
    """In place on the device, no synchronisation; d_verdict -> four device uint32: [0] header differs, [1] uncorrectable blocks,
    [2] blocks changed, [3] bytes changed."""
    _chk(lib().t3hip_repair_frame_async(C.c_void_p(d_io), C.c_uint64(n_in), C.byref(cfg) if cfg is not None else None, C.c_uint64(n_raw), C.c_uint32(flags),
                                        C.c_void_p(d_verdict), C.c_void_p(stream)), "t3hip_repair_frame_async")


def repair_profile_dev(d_io, n_in, seen, flags=REPAIR_WRITE, stream=0):
    """Header parsed (and repaired) on the host, body repaired in place, synchronises.  Returns (rc, counts): rc is OK, E_RS (some block
    uncorrectable; the rest is repaired) or E_HEADER (nothing written); counts = [header rewritten, uncorrectable blocks, blocks
    changed, bytes changed].  Other codes raise."""
    cnt = (C.c_uint32 * 4)()
    rc = lib().t3hip_repair_profile_dev(C.c_void_p(d_io), C.c_uint64(n_in), C.byref(seen), C.c_uint32(flags), cnt, C.c_void_p(stream))
    if rc not in (OK, E_HEADER, E_RS):
        raise T3Error(rc, "t3hip_repair_profile_dev")
    return rc, list(cnt)


def repair_profile(words, ctx, flags=REPAIR_WRITE):
    """Host words (n, 9) uint8, repaired IN PLACE (the array must be writable and contiguous) -> (rc, counts) as repair_profile_dev;
    ctx: a DecoderContext with mode FIXED."""
    w = words if isinstance(words, np.ndarray) and words.dtype == np.uint8 and words.flags.c_contiguous and words.flags.writeable else None
    if w is None:
        raise ValueError("repair_profile: a writable C-contiguous uint8 array (it is repaired in place)")
    if w.size % 9:
        raise ValueError("repair_profile: %d bytes are not whole words" % w.size)
    cnt = (C.c_uint32 * 4)()
    rc = lib().t3hip_repair_profile(_vp(w), C.c_uint64(w.size // 9), C.byref(ctx.cfg_last_seen), C.c_uint32(flags), cnt)
    if rc not in (OK, E_HEADER, E_RS):
        raise T3Error(rc, "t3hip_repair_profile")
    return rc, list(cnt)


# ---- repair with erasures: received bytes above 26 are known-bad positions, 2 e + s <= r (include/t3hip.h) ----------------------------
def repair_erasures_frame_async(d_io, n_in, cfg, n_raw, flags, d_verdict, stream=0):
    """repair_frame_async with bytes above 26 taken as erasures; d_verdict -> SIX device uint32: [0..3] as there, [4] body blocks holding
    a byte above 26, [5] those of them accepted."""
    _chk(lib().t3hip_repair_erasures_frame_async(C.c_void_p(d_io), C.c_uint64(n_in), C.byref(cfg) if cfg is not None else None, C.c_uint64(n_raw),
                                                 C.c_uint32(flags), C.c_void_p(d_verdict), C.c_void_p(stream)), "t3hip_repair_erasures_frame_async")


def repair_erasures_profile_dev(d_io, n_in, seen, flags=REPAIR_WRITE, stream=0):
    """repair_profile_dev with erasures -> (rc, six counts)."""
    cnt = (C.c_uint32 * 6)()
    rc = lib().t3hip_repair_erasures_profile_dev(C.c_void_p(d_io), C.c_uint64(n_in), C.byref(seen), C.c_uint32(flags), cnt, C.c_void_p(stream))
    if rc not in (OK, E_HEADER, E_RS):
        raise T3Error(rc, "t3hip_repair_erasures_profile_dev")
    return rc, list(cnt)


def repair_erasures_profile(words, ctx, flags=REPAIR_WRITE):
    """repair_profile with erasures: host words (n, 9) uint8, repaired IN PLACE -> (rc, six counts)."""
    w = words if isinstance(words, np.ndarray) and words.dtype == np.uint8 and words.flags.c_contiguous and words.flags.writeable else None
    if w is None:
        raise ValueError("repair_erasures_profile: a writable C-contiguous uint8 array (it is repaired in place)")
    if w.size % 9:
        raise ValueError("repair_erasures_profile: %d bytes are not whole words" % w.size)
    cnt = (C.c_uint32 * 6)()
    rc = lib().t3hip_repair_erasures_profile(_vp(w), C.c_uint64(w.size // 9), C.byref(ctx.cfg_last_seen), C.c_uint32(flags), cnt)
    if rc not in (OK, E_HEADER, E_RS):
        raise T3Error(rc, "t3hip_repair_erasures_profile")
    return rc, list(cnt)


# ---- decode with erasures: bytes above 26 as known-bad positions, the input read-only (include/t3hip.h) --------------------------------
class DecodeErasuresPlan(C.Structure):
    """t3_decode_erasures_plan: path 1 one launch of the fused erasure decoder, 0 private copy + erasure repair + the plain decoder."""
    _fields_ = [("path", C.c_uint8), ("pad_", C.c_uint8 * 3), ("n_tiles", C.c_uint32), ("in_bytes", C.c_uint64), ("out_units", C.c_uint64),
                ("scratch_bytes", C.c_uint64)]


FMT_WORDS, FMT_PIXELS, FMT_RGB = 0, 1, 2                # `fmt` of the erasure decoders (and of the batch entries)


def decode_erasures_plan(n_raw_words, cfg, fmt):  # host only
    p = DecodeErasuresPlan()
    _chk(lib().t3hip_decode_erasures_plan(C.c_uint64(n_raw_words), C.byref(cfg) if cfg is not None else None, C.c_int(fmt), C.byref(p)), "t3hip_decode_erasures_plan")
    return p


def decode_erasures_frame_async(d_in, n_in, cfg, n_raw, d_out, cap_units, fmt, d_verdict, stream=0):
    """decode_frame_async with bytes above 26 taken as erasures; the input is never written, no synchronisation; d_verdict -> FOUR device
    uint32: [0] header differs, [1] refused blocks, [2] body blocks holding a byte above 26, [3] those of them accepted.  Returns the
    unit count the launch will produce."""
    n = C.c_uint64()
    _chk(lib().t3hip_decode_erasures_frame_async(C.c_void_p(d_in), C.c_uint64(n_in), C.byref(cfg) if cfg is not None else None, C.c_uint64(n_raw), C.c_void_p(d_out),
                                                 C.c_uint64(cap_units), C.byref(n), C.c_int(fmt), C.c_void_p(d_verdict), C.c_void_p(stream)),
         "t3hip_decode_erasures_frame_async", n)
    return n.value


def decode_erasures_profile_dev(d_in, n_in, seen, d_out, cap_units, fmt, stream=0):
    """Header parsed on the host, body decoded with erasures, synchronises.  Returns (rc, n_out, counts): rc is OK, E_RS (some block
    refused; the output is written all the same) or E_HEADER (nothing written); counts = the four words, [0] always 0.  Other codes raise."""
    n = C.c_uint64(); cnt = (C.c_uint32 * 4)()
    rc = lib().t3hip_decode_erasures_profile_dev(C.c_void_p(d_in), C.c_uint64(n_in), C.byref(seen), C.c_void_p(d_out), C.c_uint64(cap_units), C.byref(n), C.c_int(fmt), cnt,
                                                 C.c_void_p(stream))
    if rc not in (OK, E_HEADER, E_RS):
        raise T3Error(rc, "t3hip_decode_erasures_profile_dev", n.value)
    return rc, n.value, list(cnt)


def decode_erasures_profile(words, ctx, fmt):
    """Host words (n, 9) uint8, never written -> (rc, output, counts) as decode_erasures_profile_dev; output: (n, 9) uint8 words (fmt 0),
    PIXEL_DT pixels (fmt 1) or (n, 3) uint8 RGB (fmt 2), empty on E_HEADER; ctx: a DecoderContext with mode FIXED."""
    w = np.ascontiguousarray(words, np.uint8).reshape(-1)
    if w.size % 9:
        raise ValueError("decode_erasures_profile: %d bytes are not whole words" % w.size)
    n_in = w.size // 9
    size = {FMT_WORDS: 9, FMT_PIXELS: 6, FMT_RGB: 3}[fmt]
    cap = 2 * n_in
    out = np.zeros(cap * size, np.uint8)
    n = C.c_uint64(); cnt = (C.c_uint32 * 4)()
    rc = lib().t3hip_decode_erasures_profile(_vp(w), C.c_uint64(n_in), C.byref(ctx.cfg_last_seen), _vp(out), C.c_uint64(cap), C.byref(n), C.c_int(fmt), cnt)
    if rc not in (OK, E_HEADER, E_RS):
        raise T3Error(rc, "t3hip_decode_erasures_profile", n.value)
    got = out[: n.value * size] if rc != E_HEADER else out[:0]
    return rc, (got.view(PIXEL_DT) if fmt == FMT_PIXELS else got.reshape(-1, size)), list(cnt)


def rs_decode_block_erasures_host(k, code26):
    """One block on the host, no device: 26 bytes, those above 26 are erasures -> (accepted, the 26 bytes afterwards, the k data symbols or
    None).  A refused block comes back untouched."""
    c = np.ascontiguousarray(code26, np.uint8).reshape(26).copy()
    d = np.zeros(max(int(k), 1), np.uint8)
    rc = lib().t3hip_rs_decode_block_erasures_host(C.c_int(k), _vp(c), _vp(d))
    if rc not in (0, 1):
        raise T3Error(rc, "t3hip_rs_decode_block_erasures_host")
    return rc == 1, c, (d[:k] if rc == 1 else None)


def rs_decode_blocks_erasures_dev(k, d_code, n_blocks, d_data, d_ok, stream=0):
    _chk(lib().t3hip_rs_decode_blocks_erasures_dev(C.c_int(k), C.c_void_p(d_code), C.c_uint64(n_blocks), C.c_void_p(d_data), C.c_void_p(d_ok), C.c_void_p(stream)),
         "t3hip_rs_decode_blocks_erasures_dev")


def rs_decode_blocks_erasures(k, code26, data_k=None):
    """Host blocks (n, 26) uint8 -> (the blocks afterwards, data (n, k), ok (n,)); data rows of refused blocks are data_k's (zeros if None)."""
    c = np.ascontiguousarray(code26, np.uint8).reshape(-1, 26).copy()
    n = len(c)
    d = np.zeros((n, k), np.uint8) if data_k is None else np.ascontiguousarray(data_k, np.uint8).reshape(n, k).copy()
    ok = np.zeros(n, np.uint8)
    _chk(lib().t3hip_rs_decode_blocks_erasures(C.c_int(k), _vp(c), C.c_uint64(n), _vp(d), _vp(ok)), "t3hip_rs_decode_blocks_erasures")
    return c, d, ok


# ---- repair of a batch of equal FIXED frames in place: frame f lies f * stride bytes behind frame 0 (include/t3hip.h) --------------------
class RepairFramesPlan(C.Structure):
    """t3_repair_frames_plan: one frame's repair plan (path, tiles), whether the batch runs as ONE repair launch over all frames or as a
    loop of the single-frame body, the coded bytes of one frame and the smallest (even) stride."""
    _fields_ = [("n_frames", C.c_uint32), ("tiles_per_frame", C.c_uint32), ("one_launch", C.c_uint8), ("path", C.c_uint8), ("pad_", C.c_uint8 * 6),
                ("in_bytes", C.c_uint64), ("stride_min", C.c_uint64)]


def repair_frames_plan(n_raw_words, n_frames, cfg):  # host only
    p = RepairFramesPlan()
    _chk(lib().t3hip_repair_frames_plan(C.c_uint64(n_raw_words), C.c_uint32(n_frames), C.byref(cfg) if cfg is not None else None, C.byref(p)),
         "t3hip_repair_frames_plan")
    return p


def repair_frames_async(d_io, n_in, stride, n_frames, cfg, n_raw, flags, d_verdict, stream=0):
    """In place on the device, no synchronisation; even base, even stride >= 9 * n_in; d_verdict -> 4 * n_frames device uint32, the four
    words of repair_frame_async per frame."""
    _chk(lib().t3hip_repair_frames_async(C.c_void_p(d_io), C.c_uint64(n_in), C.c_uint64(stride), C.c_uint32(n_frames), C.byref(cfg) if cfg is not None else None,
                                         C.c_uint64(n_raw), C.c_uint32(flags), C.c_void_p(d_verdict), C.c_void_p(stream)), "t3hip_repair_frames_async")


def repair_frames_dev(d_io, n_in, stride, n_frames, seen, flags=REPAIR_WRITE, stream=0):
    """Every frame's header parsed (and repaired) on the host, the bodies repaired in place by one batched launch per run of equal
    headers, synchronises.  Returns (rc, [rc per frame: OK / E_RS / E_HEADER], [counts per frame, as repair_profile_dev]); rc is OK, or
    E_HEADER when no frame's header decodes.  Other codes raise."""
    return _repair_frames_dev("t3hip_repair_frames_dev", 4, d_io, n_in, stride, n_frames, seen, flags, stream)


def _repair_frames_dev(entry, nw, d_io, n_in, stride, n_frames, seen, flags, stream):
    """The _dev batch entries: nw = 4 (plain) or 6 (erasures) counts per frame"""
    cnt = (C.c_uint32 * (nw * n_frames))(); rcs = (C.c_int * n_frames)()
    rc = getattr(lib(), entry)(C.c_void_p(d_io), C.c_uint64(n_in), C.c_uint64(stride), C.c_uint32(n_frames), C.byref(seen), C.c_uint32(flags), cnt, rcs,
                               C.c_void_p(stream))
    if rc not in (OK, E_HEADER):
        raise T3Error(rc, entry)
    return rc, list(rcs), [list(cnt[nw * f: nw * f + nw]) for f in range(n_frames)]


def repair_frames(words, ctx, flags=REPAIR_WRITE, stride=None):
    """Host frames repaired IN PLACE: `words` a writable C-contiguous uint8 array of shape (n_frames, stride), each row a frame's coded
    words and whatever pads the stride (never read or written), or a flat array plus `stride` (the last frame may end with its words).
    The frame is the largest whole number of words a row holds.  -> (rc, [rc per frame], [counts per frame]) as repair_frames_dev; ctx: a
    DecoderContext with mode FIXED."""
    return _repair_frames("repair_frames", 4, words, ctx, flags, stride)


def _repair_frames(name, nw, words, ctx, flags, stride):
    """The host batch entries: nw = 4 (plain) or 6 (erasures) counts per frame"""
    w = words if isinstance(words, np.ndarray) and words.dtype == np.uint8 and words.flags.c_contiguous and words.flags.writeable else None
    if w is None:
        raise ValueError("%s: a writable C-contiguous uint8 array (it is repaired in place)" % name)
    if stride is None:
        if w.ndim != 2:
            raise ValueError("%s: an array of shape (n_frames, stride), or a flat array and a stride" % name)
        n_frames, stride = int(w.shape[0]), int(w.shape[1])
    else:
        stride = int(stride)
        if w.ndim != 1 or stride <= 0:
            raise ValueError("%s: a flat array with a positive stride" % name)
        n_frames = -(-w.size // stride)
    if n_frames == 0:
        return OK, [], []
    n_in = min(stride, w.size - (n_frames - 1) * stride) // 9
    cnt = (C.c_uint32 * (nw * n_frames))(); rcs = (C.c_int * n_frames)()
    rc = getattr(lib(), "t3hip_" + name)(_vp(w), C.c_uint64(n_in), C.c_uint64(stride), C.c_uint32(n_frames), C.byref(ctx.cfg_last_seen), C.c_uint32(flags), cnt, rcs)
    if rc not in (OK, E_HEADER):
        raise T3Error(rc, "t3hip_" + name)
    return rc, list(rcs), [list(cnt[nw * f: nw * f + nw]) for f in range(n_frames)]


# ---- repair with erasures of a batch of equal FIXED frames in place: six words per frame (include/t3hip.h) ---------------------------------
def repair_erasures_frames_async(d_io, n_in, stride, n_frames, cfg, n_raw, flags, d_verdict, stream=0):
    """repair_frames_async with bytes above 26 taken as erasures; d_verdict -> 6 * n_frames device uint32, the six words of
    repair_erasures_frame_async per frame.  repair_frames_plan serves unchanged."""
    _chk(lib().t3hip_repair_erasures_frames_async(C.c_void_p(d_io), C.c_uint64(n_in), C.c_uint64(stride), C.c_uint32(n_frames),
                                                  C.byref(cfg) if cfg is not None else None, C.c_uint64(n_raw), C.c_uint32(flags), C.c_void_p(d_verdict),
                                                  C.c_void_p(stream)), "t3hip_repair_erasures_frames_async")


def repair_erasures_frames_dev(d_io, n_in, stride, n_frames, seen, flags=REPAIR_WRITE, stream=0):
    """repair_frames_dev with erasures -> (rc, [rc per frame], [six counts per frame, as repair_erasures_profile_dev])."""
    return _repair_frames_dev("t3hip_repair_erasures_frames_dev", 6, d_io, n_in, stride, n_frames, seen, flags, stream)


def repair_erasures_frames(words, ctx, flags=REPAIR_WRITE, stride=None):
    """repair_frames with erasures: host frames (n_frames, stride) or a flat array plus `stride`, repaired IN PLACE -> (rc, [rc per
    frame], [six counts per frame])."""
    return _repair_frames("repair_erasures_frames", 6, words, ctx, flags, stride)


# ---- decode with erasures of a batch of equal FIXED frames, the input read-only: four words per frame (include/t3hip.h) -------------------
class DecodeErasuresFramesPlan(C.Structure):
    """t3_decode_erasures_frames_plan: one frame's plan, whether the batch runs as ONE launch of the fused erasure decoder over all frames
    or as a loop of the single-frame body, the stride minima and the per-stream scratch the call holds."""
    _fields_ = [("frame", DecodeErasuresPlan), ("n_frames", C.c_uint32), ("one_launch", C.c_uint8), ("pad_", C.c_uint8 * 3), ("in_stride_min", C.c_uint64),
                ("out_bytes", C.c_uint64), ("out_stride_min", C.c_uint64), ("scratch_bytes", C.c_uint64)]


def decode_erasures_frames_plan(n_raw_words, n_frames, cfg, fmt):  # host only
    p = DecodeErasuresFramesPlan()
    _chk(lib().t3hip_decode_erasures_frames_plan(C.c_uint64(n_raw_words), C.c_uint32(n_frames), C.byref(cfg) if cfg is not None else None, C.c_int(fmt), C.byref(p)),
         "t3hip_decode_erasures_frames_plan")
    return p


def decode_erasures_frames_async(d_in, n_in, in_stride, n_frames, cfg, n_raw, d_out, out_stride, fmt, d_verdict, stream=0):
    """decode_frames_async with bytes above 26 taken as erasures; the input is never written, no synchronisation; even input base and
    stride, 16-byte output base and stride; d_verdict -> 4 * n_frames device uint32, the four words of decode_erasures_frame_async per
    frame."""
    _chk(lib().t3hip_decode_erasures_frames_async(C.c_void_p(d_in), C.c_uint64(n_in), C.c_uint64(in_stride), C.c_uint32(n_frames), C.byref(cfg) if cfg is not None else None,
                                                  C.c_uint64(n_raw), C.c_void_p(d_out), C.c_uint64(out_stride), C.c_int(fmt), C.c_void_p(d_verdict), C.c_void_p(stream)),
         "t3hip_decode_erasures_frames_async")


def decode_erasures_frames_dev(d_in, n_in, in_stride, n_frames, seen, d_out, out_stride, cap_units, fmt, stream=0):
    """Every frame's header parsed on the host, the bodies decoded with erasures by one batched launch per run of equal headers,
    synchronises.  Returns (rc, n_out, [rc per frame: OK / E_RS / E_HEADER / E_CAPACITY], [four counts per frame, [0] always 0]); rc is OK,
    or E_HEADER when no frame's header decodes; n_out: units of one frame.  Other codes raise."""
    n = C.c_uint64(); cnt = (C.c_uint32 * (4 * n_frames))(); rcs = (C.c_int * n_frames)()
    rc = lib().t3hip_decode_erasures_frames_dev(C.c_void_p(d_in), C.c_uint64(n_in), C.c_uint64(in_stride), C.c_uint32(n_frames), C.byref(seen), C.c_void_p(d_out),
                                                C.c_uint64(out_stride), C.c_uint64(cap_units), C.byref(n), C.c_int(fmt), cnt, rcs, C.c_void_p(stream))
    if rc not in (OK, E_HEADER):
        raise T3Error(rc, "t3hip_decode_erasures_frames_dev", n.value)
    return rc, n.value, list(rcs), [list(cnt[4 * f: 4 * f + 4]) for f in range(n_frames)]


def decode_erasures_frames(words, ctx, fmt, stride=None):
    """Host frames, never written: `words` a C-contiguous uint8 array of shape (n_frames, stride), each row a frame's coded words and
    whatever pads the stride, or a flat array plus `stride` (the last frame may end with its words), as repair_erasures_frames takes
    them.  -> (rc, [rc per frame], [output per frame], [four counts per frame]) as decode_erasures_frames_dev; an output is (n, 9) uint8
    words (fmt 0), PIXEL_DT pixels (fmt 1) or (n, 3) uint8 RGB (fmt 2), empty for a frame that is neither OK nor E_RS; ctx: a
    DecoderContext with mode FIXED."""
    w = np.ascontiguousarray(words, np.uint8)
    if stride is None:
        if w.ndim != 2:
            raise ValueError("decode_erasures_frames: an array of shape (n_frames, stride), or a flat array and a stride")
        n_frames, stride = int(w.shape[0]), int(w.shape[1])
    else:
        stride = int(stride)
        if w.ndim != 1 or stride <= 0:
            raise ValueError("decode_erasures_frames: a flat array with a positive stride")
        n_frames = -(-w.size // stride)
    if n_frames == 0:
        return OK, [], [], []
    n_in = min(stride, w.size - (n_frames - 1) * stride) // 9
    size = {FMT_WORDS: 9, FMT_PIXELS: 6, FMT_RGB: 3}[fmt]
    cap = 2 * n_in
    out = np.zeros((n_frames, cap * size), np.uint8)
    n = C.c_uint64(); cnt = (C.c_uint32 * (4 * n_frames))(); rcs = (C.c_int * n_frames)()
    rc = lib().t3hip_decode_erasures_frames(_vp(w), C.c_uint64(n_in), C.c_uint64(stride), C.c_uint32(n_frames), C.byref(ctx.cfg_last_seen), _vp(out),
                                            C.c_uint64(cap * size), C.c_uint64(cap), C.byref(n), C.c_int(fmt), cnt, rcs)
    if rc not in (OK, E_HEADER):
        raise T3Error(rc, "t3hip_decode_erasures_frames", n.value)
    units = []
    for f in range(n_frames):
        b = out[f, : n.value * size] if rc == OK and rcs[f] in (OK, E_RS) else out[f, :0]
        units.append(b.view(PIXEL_DT).copy() if fmt == FMT_PIXELS else b.reshape(-1, size).copy())
    return rc, list(rcs), units, [list(cnt[4 * f: 4 * f + 4]) for f in range(n_frames)]


# ---- decode a window with erasures: a pixel window of a FIXED frame straight from its tiles, the input read-only (include/t3hip.h) -------
class DecodeErasuresWindowPlan(C.Structure):
    """t3_decode_erasures_window_plan: the window plan of the same arguments, the erasure plan's path (1: ONE launch of decode_era_window_px,
    0: private copy + erasure repair + window decode of the copy), whether the output is zeroed first, and what the call launches and holds."""
    _fields_ = [("win", WindowPlan), ("path", C.c_uint8), ("zero_fill", C.c_uint8), ("pad_", C.c_uint8 * 2), ("tiles_launched", C.c_uint32),
                ("in_bytes", C.c_uint64), ("out_bytes", C.c_uint64), ("scratch_bytes", C.c_uint64)]


def decode_erasures_window_plan(n_raw_words, cfg, fw, fh, x0, y0, w, h, out_fmt):  # host only
    p = DecodeErasuresWindowPlan()
    _chk(lib().t3hip_decode_erasures_window_plan(C.c_uint64(n_raw_words), C.byref(cfg) if cfg is not None else None, C.c_uint32(fw), C.c_uint32(fh), C.c_uint32(x0),
                                                 C.c_uint32(y0), C.c_uint32(w), C.c_uint32(h), C.c_int(out_fmt), C.byref(p)), "t3hip_decode_erasures_window_plan")
    return p


def decode_erasures_window_async(d_in, n_in, cfg, n_raw, fw, fh, x0, y0, w, h, d_out, out_fmt, d_verdict, stream=0):
    """decode_window_async with bytes above 26 taken as erasures; the input is never written, no synchronisation; d_out 4-byte aligned,
    w * h * (6 | 3) bytes; d_verdict -> FOUR device uint32, the words of decode_erasures_frame_async counted among the decoded blocks."""
    _chk(lib().t3hip_decode_erasures_window_async(C.c_void_p(d_in), C.c_uint64(n_in), C.byref(cfg) if cfg is not None else None, C.c_uint64(n_raw), C.c_uint32(fw),
                                                  C.c_uint32(fh), C.c_uint32(x0), C.c_uint32(y0), C.c_uint32(w), C.c_uint32(h), C.c_void_p(d_out), C.c_int(out_fmt),
                                                  C.c_void_p(d_verdict), C.c_void_p(stream)), "t3hip_decode_erasures_window_async")


def decode_erasures_window_dev(d_in, n_in, seen, fw, fh, x0, y0, w, h, d_out, out_fmt, stream=0):
    """Header parsed on the host, the window decoded with erasures, synchronises.  Returns (rc, counts): rc is OK, E_RS (some decoded block
    refused; the window is written all the same) or E_HEADER (nothing written); counts = the four words, [0] always 0.  Other codes raise."""
    cnt = (C.c_uint32 * 4)()
    rc = lib().t3hip_decode_erasures_window_dev(C.c_void_p(d_in), C.c_uint64(n_in), C.byref(seen), C.c_uint32(fw), C.c_uint32(fh), C.c_uint32(x0), C.c_uint32(y0),
                                                C.c_uint32(w), C.c_uint32(h), C.c_void_p(d_out), C.c_int(out_fmt), cnt, C.c_void_p(stream))
    if rc not in (OK, E_HEADER, E_RS):
        raise T3Error(rc, "t3hip_decode_erasures_window_dev")
    return rc, list(cnt)


def decode_erasures_window(words, ctx, fw, fh, x0, y0, w, h, out_fmt):
    """Host words (n, 9) uint8, never written -> (rc, window, counts) as decode_erasures_window_dev; window: (h, w) PIXEL_DT pixels
    (WINDOW_PIXELS) or (h, w, 3) uint8 RGB (WINDOW_RGB), None on E_HEADER; ctx: a DecoderContext with mode FIXED."""
    wd = np.ascontiguousarray(words, np.uint8).reshape(-1)
    if wd.size % 9:
        raise ValueError("decode_erasures_window: %d bytes are not whole words" % wd.size)
    size = {WINDOW_PIXELS: 6, WINDOW_RGB: 3}[out_fmt]
    out = np.zeros(int(w) * int(h) * size, np.uint8)
    cnt = (C.c_uint32 * 4)()
    rc = lib().t3hip_decode_erasures_window(_vp(wd), C.c_uint64(wd.size // 9), C.byref(ctx.cfg_last_seen), C.c_uint32(fw), C.c_uint32(fh), C.c_uint32(x0), C.c_uint32(y0),
                                            C.c_uint32(w), C.c_uint32(h), _vp(out), C.c_int(out_fmt), cnt)
    if rc not in (OK, E_HEADER, E_RS):
        raise T3Error(rc, "t3hip_decode_erasures_window")
    if rc == E_HEADER:
        return rc, None, list(cnt)
    return rc, (out.view(PIXEL_DT).reshape(h, w) if out_fmt == WINDOW_PIXELS else out.reshape(h, w, 3)), list(cnt)


# ---- decode a window with erasures of a batch of equal FIXED frames: the same window of every frame, the input read-only (include/t3hip.h) --
class DecodeErasuresFramesWindowPlan(C.Structure):
    """t3_decode_erasures_frames_window_plan: one frame's window plan, whether the batch runs as ONE launch of decode_era_frames_window_px
    over the window's tiles of all frames or as a loop of the single-frame window body, the tickets of that launch, the stride minima and
    the per-stream scratch the call holds."""
    _fields_ = [("frame", DecodeErasuresWindowPlan), ("n_frames", C.c_uint32), ("one_launch", C.c_uint8), ("pad_", C.c_uint8 * 3), ("tiles_launched", C.c_uint32),
                ("pad2_", C.c_uint32), ("in_stride_min", C.c_uint64), ("out_bytes", C.c_uint64), ("out_stride_min", C.c_uint64), ("scratch_bytes", C.c_uint64)]


def decode_erasures_frames_window_plan(n_raw_words, n_frames, cfg, fw, fh, x0, y0, w, h, out_fmt):  # host only
    p = DecodeErasuresFramesWindowPlan()
    _chk(lib().t3hip_decode_erasures_frames_window_plan(C.c_uint64(n_raw_words), C.c_uint32(n_frames), C.byref(cfg) if cfg is not None else None, C.c_uint32(fw), C.c_uint32(fh),
                                                        C.c_uint32(x0), C.c_uint32(y0), C.c_uint32(w), C.c_uint32(h), C.c_int(out_fmt), C.byref(p)),
         "t3hip_decode_erasures_frames_window_plan")
    return p


def decode_erasures_frames_window_async(d_in, n_in, in_stride, n_frames, cfg, n_raw, fw, fh, x0, y0, w, h, d_out, out_stride, out_fmt, d_verdict, stream=0):
    """decode_erasures_window_async on every frame of a batch in one call; the input is never written, no synchronisation; even input
    base and stride, 16-byte output base and stride; d_verdict -> 4 * n_frames device uint32, the four words of
    decode_erasures_window_async per frame."""
    _chk(lib().t3hip_decode_erasures_frames_window_async(C.c_void_p(d_in), C.c_uint64(n_in), C.c_uint64(in_stride), C.c_uint32(n_frames), C.byref(cfg) if cfg is not None else None,
                                                         C.c_uint64(n_raw), C.c_uint32(fw), C.c_uint32(fh), C.c_uint32(x0), C.c_uint32(y0), C.c_uint32(w), C.c_uint32(h),
                                                         C.c_void_p(d_out), C.c_uint64(out_stride), C.c_int(out_fmt), C.c_void_p(d_verdict), C.c_void_p(stream)),
         "t3hip_decode_erasures_frames_window_async")


def decode_erasures_frames_window_dev(d_in, n_in, in_stride, n_frames, seen, fw, fh, x0, y0, w, h, d_out, out_stride, out_fmt, stream=0):
    """Every frame's header parsed on the host, the window of every frame decoded with erasures by one batched launch per run of equal
    headers, synchronises.  Returns (rc, [rc per frame: OK / E_RS / E_HEADER], [four counts per frame, [0] always 0]); rc is OK, or
    E_HEADER when no frame's header decodes.  Other codes raise."""
    cnt = (C.c_uint32 * (4 * n_frames))(); rcs = (C.c_int * n_frames)()
    rc = lib().t3hip_decode_erasures_frames_window_dev(C.c_void_p(d_in), C.c_uint64(n_in), C.c_uint64(in_stride), C.c_uint32(n_frames), C.byref(seen), C.c_uint32(fw),
                                                       C.c_uint32(fh), C.c_uint32(x0), C.c_uint32(y0), C.c_uint32(w), C.c_uint32(h), C.c_void_p(d_out), C.c_uint64(out_stride),
                                                       C.c_int(out_fmt), cnt, rcs, C.c_void_p(stream))
    if rc not in (OK, E_HEADER):
        raise T3Error(rc, "t3hip_decode_erasures_frames_window_dev")
    return rc, list(rcs), [list(cnt[4 * f: 4 * f + 4]) for f in range(n_frames)]


def decode_erasures_frames_window(words, ctx, fw, fh, x0, y0, w, h, out_fmt, stride=None):
    """Host frames, never written: `words` a C-contiguous uint8 array of shape (n_frames, stride) or a flat array plus `stride`, as
    decode_erasures_frames takes them.  -> (rc, [rc per frame], [window per frame], [four counts per frame]) as
    decode_erasures_frames_window_dev; a window is (h, w) PIXEL_DT pixels (WINDOW_PIXELS) or (h, w, 3) uint8 RGB (WINDOW_RGB), None for a
    frame that is neither OK nor E_RS; ctx: a DecoderContext with mode FIXED."""
    wd = np.ascontiguousarray(words, np.uint8)
    if stride is None:
        if wd.ndim != 2:
            raise ValueError("decode_erasures_frames_window: an array of shape (n_frames, stride), or a flat array and a stride")
        n_frames, stride = int(wd.shape[0]), int(wd.shape[1])
    else:
        stride = int(stride)
        if wd.ndim != 1 or stride <= 0:
            raise ValueError("decode_erasures_frames_window: a flat array with a positive stride")
        n_frames = -(-wd.size // stride)
    if n_frames == 0:
        return OK, [], [], []
    n_in = min(stride, wd.size - (n_frames - 1) * stride) // 9
    size = {WINDOW_PIXELS: 6, WINDOW_RGB: 3}[out_fmt]
    ob = int(w) * int(h) * size
    out = np.zeros((n_frames, ob), np.uint8)
    cnt = (C.c_uint32 * (4 * n_frames))(); rcs = (C.c_int * n_frames)()
    rc = lib().t3hip_decode_erasures_frames_window(_vp(wd), C.c_uint64(n_in), C.c_uint64(stride), C.c_uint32(n_frames), C.byref(ctx.cfg_last_seen), C.c_uint32(fw),
                                                   C.c_uint32(fh), C.c_uint32(x0), C.c_uint32(y0), C.c_uint32(w), C.c_uint32(h), _vp(out), C.c_uint64(ob), C.c_int(out_fmt),
                                                   cnt, rcs)
    if rc not in (OK, E_HEADER):
        raise T3Error(rc, "t3hip_decode_erasures_frames_window")
    wins = []
    for f in range(n_frames):
        if rc != OK or rcs[f] not in (OK, E_RS):
            wins.append(None)
        else:
            wins.append(out[f].view(PIXEL_DT).reshape(h, w).copy() if out_fmt == WINDOW_PIXELS else out[f].reshape(h, w, 3).copy())
    return rc, list(rcs), wins, [list(cnt[4 * f: 4 * f + 4]) for f in range(n_frames)]


# ---- batches of equal frames: N frames of one configuration and size in one call (include/t3hip.h) --------------------------
class FramesPlan(C.Structure):
    """t3_frames_plan: how a batch call runs -- one codec launch over all frames, or a loop of the single-frame path -- and the
    bytes and minimum strides of one frame."""
    _fields_ = [("n_frames", C.c_uint32), ("tiles_per_frame", C.c_uint32), ("one_launch", C.c_uint8), ("pad_", C.c_uint8 * 7),
                ("in_bytes", C.c_uint64), ("out_bytes", C.c_uint64), ("in_stride_min", C.c_uint64), ("out_stride_min", C.c_uint64)]


FRAMES_WORDS, FRAMES_PIXELS, FRAMES_RGB = 0, 1, 2       # the unit side of a batch call: raw Word27 (9 B), PixelYCbCrQuant (6 B), RGB8 (3 B)
_FRAMES_UNIT = {FRAMES_WORDS: 9, FRAMES_PIXELS: 6, FRAMES_RGB: 3}


def frames_plan(decode, n_units, n_frames, cfg, fmt=FRAMES_PIXELS):  # host only
    p = FramesPlan()
    _chk(lib().t3hip_frames_plan(C.c_int(1 if decode else 0), C.c_uint64(n_units), C.c_uint32(n_frames), C.byref(cfg) if cfg is not None else None,
                                 C.c_int(fmt), C.byref(p)), "t3hip_frames_plan")
    return p


def encode_frames_dev(d_in, n_units, fmt, in_stride, n_frames, cfg, d_out, out_stride, stream=0):
    """n_frames frames of n_units units each, frame f at d_in + f * in_stride -> coded streams at d_out + f * out_stride (16-byte aligned
    bases and strides); returns the coded word count of one frame."""
    n = C.c_uint64()
    _chk(lib().t3hip_encode_frames_dev(C.c_void_p(d_in), C.c_uint64(n_units), C.c_int(fmt), C.c_uint64(in_stride), C.c_uint32(n_frames), C.byref(cfg),
                                       C.c_void_p(d_out), C.c_uint64(out_stride), C.byref(n), C.c_void_p(stream)), "t3hip_encode_frames_dev")
    return n.value


def decode_frames_async(d_in, n_in, in_stride, n_frames, cfg, n_raw, d_out, out_stride, fmt, d_verdict, stream=0):
    """Streaming decode of a batch with a known configuration, no synchronisation; d_verdict -> 2 * n_frames device uint32, the two words
    of decode_frame_async per frame."""
    _chk(lib().t3hip_decode_frames_async(C.c_void_p(d_in), C.c_uint64(n_in), C.c_uint64(in_stride), C.c_uint32(n_frames), C.byref(cfg), C.c_uint64(n_raw),
                                         C.c_void_p(d_out), C.c_uint64(out_stride), C.c_int(fmt), C.c_void_p(d_verdict), C.c_void_p(stream)), "t3hip_decode_frames_async")


def _round16(x):
    return (x + 15) & ~15


def encode_frames(frames, ectx, fmt=FRAMES_PIXELS):
    """Equal frames (a sequence of unit arrays) -> (True, [coded words per frame]); ValueError for frames of unequal size."""
    cfg = ectx.cfg if isinstance(ectx, EncoderContext) else ectx
    dt = PIXEL_DT if fmt == FRAMES_PIXELS else np.uint8
    fr = [np.ascontiguousarray(f, dt).reshape(-1) if fmt == FRAMES_PIXELS else np.ascontiguousarray(f, dt).reshape(-1, _FRAMES_UNIT[fmt]) for f in frames]
    if not fr:
        return True, []
    if any(len(f) != len(fr[0]) for f in fr):
        raise ValueError("encode_frames: frames of unequal size")
    n_units = len(fr[0])
    p = frames_plan(False, n_units, len(fr), cfg, fmt)
    src = np.zeros((len(fr), p.in_stride_min), np.uint8); out = np.zeros((len(fr), p.out_stride_min), np.uint8)
    for i, f in enumerate(fr):
        src[i, : p.in_bytes] = f.view(np.uint8).reshape(-1)
    n = C.c_uint64()
    _chk(lib().t3hip_encode_frames(_vp(src), C.c_uint64(n_units), C.c_int(fmt), C.c_uint64(p.in_stride_min), C.c_uint32(len(fr)), C.byref(cfg),
                                   _vp(out), C.c_uint64(p.out_stride_min), C.byref(n)), "t3hip_encode_frames")
    return True, [out[i, : 9 * n.value].reshape(-1, 9).copy() for i in range(len(fr))]


def decode_frames(streams, dctx, fmt=FRAMES_PIXELS):
    """Equal coded frames (a sequence of word arrays) -> ([rc per frame: OK / E_HEADER / E_RS], [units per frame]); frame 0's header sets
    the configuration (dctx.cfg_last_seen is updated as decode_frame does for frame 0)."""
    seen = dctx.cfg_last_seen if isinstance(dctx, DecoderContext) else dctx
    ws = [np.ascontiguousarray(w, np.uint8).reshape(-1, 9) for w in streams]
    if not ws:
        return [], []
    if any(len(w) != len(ws[0]) for w in ws):
        raise ValueError("decode_frames: frames of unequal size")
    n_in, ub = len(ws[0]), _FRAMES_UNIT[fmt]
    cap = (1 if fmt == FRAMES_WORDS else 2) * (n_in + 16)
    in_stride, out_stride = _round16(9 * n_in), _round16(cap * ub)
    src = np.zeros((len(ws), in_stride), np.uint8); out = np.zeros((len(ws), out_stride), np.uint8)
    for i, w in enumerate(ws):
        src[i, : 9 * n_in] = w.reshape(-1)
    n = C.c_uint64(); rcs = (C.c_int * len(ws))()
    rc = lib().t3hip_decode_frames(_vp(src), C.c_uint64(n_in), C.c_uint64(in_stride), C.c_uint32(len(ws)), _vp(out), C.c_uint64(out_stride), C.c_uint64(cap),
                                   C.c_int(fmt), C.byref(seen), C.byref(n), rcs)
    if rc == E_HEADER:  # frame 0's header did not decode: nothing was decoded
        return [E_HEADER] * len(ws), [out[0, :0]] * len(ws)
    _chk(rc, "t3hip_decode_frames", n)
    units = []
    for i in range(len(ws)):
        b = out[i, : n.value * ub] if rcs[i] == OK else out[i, :0]
        units.append(b.view(PIXEL_DT).copy() if fmt == FRAMES_PIXELS else b.reshape(-1, ub).copy())
    return list(rcs), units



# ---- the same window out of every frame of a batch; batches through the image front end (include/t3hip.h) --------------------------------
class FramesWindowPlan(C.Structure):
    """t3_frames_window_plan: one frame's window plan, whether the batch runs as one decoder launch + one crop launch, the bytes and
    minimum strides of one frame and the per-stream scratch the call holds."""
    _fields_ = [("win", WindowPlan), ("n_frames", C.c_uint32), ("one_launch", C.c_uint8), ("pad_", C.c_uint8 * 3),
                ("in_bytes", C.c_uint64), ("out_bytes", C.c_uint64), ("in_stride_min", C.c_uint64), ("out_stride_min", C.c_uint64),
                ("scratch_bytes", C.c_uint64)]


def frames_window_plan(n_raw_words, n_frames, cfg, fw, fh, x0, y0, w, h, out_fmt=WINDOW_PIXELS):  # host only
    p = FramesWindowPlan()
    _chk(lib().t3hip_frames_window_plan(C.c_uint64(n_raw_words), C.c_uint32(n_frames), C.byref(cfg) if cfg is not None else None, C.c_uint32(fw), C.c_uint32(fh),
                                        C.c_uint32(x0), C.c_uint32(y0), C.c_uint32(w), C.c_uint32(h), C.c_int(out_fmt), C.byref(p)), "t3hip_frames_window_plan")
    return p


def decode_frames_window_async(d_in, n_in, in_stride, n_frames, cfg, n_raw, fw, fh, x0, y0, w, h, d_out, out_stride, out_fmt, d_verdict, stream=0):
    """The w x h window at (x0, y0) out of each of n_frames coded frames (frame f at d_in + f * in_stride) -> d_out + f * out_stride, no
    synchronisation; d_verdict -> 2 * n_frames device uint32, decode_window_async's two words per frame."""
    _chk(lib().t3hip_decode_frames_window_async(C.c_void_p(d_in), C.c_uint64(n_in), C.c_uint64(in_stride), C.c_uint32(n_frames), C.byref(cfg), C.c_uint64(n_raw),
                                                C.c_uint32(fw), C.c_uint32(fh), C.c_uint32(x0), C.c_uint32(y0), C.c_uint32(w), C.c_uint32(h), C.c_void_p(d_out),
                                                C.c_uint64(out_stride), C.c_int(out_fmt), C.c_void_p(d_verdict), C.c_void_p(stream)), "t3hip_decode_frames_window_async")


def decode_frames_window(streams, cfg, n_raw, fw, fh, x0, y0, w, h, out_fmt=WINDOW_PIXELS):
    """Equal coded frames (a sequence of word arrays) of a known configuration -> ([rc per frame: OK / E_RS / E_HEADER], [window per
    frame: pixel records or (w * h, 3) uint8]); a frame that did not decode comes back empty."""
    ws = [np.ascontiguousarray(x, np.uint8).reshape(-1, 9) for x in streams]
    if not ws:
        return [], []
    if any(len(x) != len(ws[0]) for x in ws):
        raise ValueError("decode_frames_window: frames of unequal size")
    n_in = len(ws[0])
    p = frames_window_plan(n_raw, len(ws), cfg, fw, fh, x0, y0, w, h, out_fmt)
    in_stride = _round16(9 * n_in)
    src = np.zeros((len(ws), in_stride), np.uint8); out = np.zeros((len(ws), max(p.out_stride_min, 16)), np.uint8)
    for i, x in enumerate(ws):
        src[i, : 9 * n_in] = x.reshape(-1)
    rcs = (C.c_int * len(ws))()
    _chk(lib().t3hip_decode_frames_window(_vp(src), C.c_uint64(n_in), C.c_uint64(in_stride), C.c_uint32(len(ws)), C.byref(cfg), C.c_uint64(n_raw), C.c_uint32(fw),
                                          C.c_uint32(fh), C.c_uint32(x0), C.c_uint32(y0), C.c_uint32(w), C.c_uint32(h), _vp(out), C.c_uint64(out.shape[1]),
                                          C.c_int(out_fmt), rcs), "t3hip_decode_frames_window")
    wins = []
    for i in range(len(ws)):
        b = out[i, : p.out_bytes] if rcs[i] == OK else out[i, :0]
        wins.append(b.view(PIXEL_DT).copy() if out_fmt == WINDOW_PIXELS else b.reshape(-1, 3).copy())
    return list(rcs), wins


def decode_images_async(d_in, n_in, in_stride, n_frames, cfg, sub, centered, d_rgb, out_stride, d_verdict, stream=0):
    """n_frames coded frames -> their target-sized RGB8 images (tw * th * 3 bytes each, image f at d_rgb + f * out_stride)."""
    _chk(lib().t3hip_decode_images_async(C.c_void_p(d_in), C.c_uint64(n_in), C.c_uint64(in_stride), C.c_uint32(n_frames), C.byref(cfg), C.c_int(int(sub)),
                                         C.c_int(1 if centered else 0), C.c_void_p(d_rgb), C.c_uint64(out_stride), C.c_void_p(d_verdict), C.c_void_p(stream)),
         "t3hip_decode_images_async")


def encode_images_dev(d_src, sw, sh, src_stride, n_frames, sub, centered, cfg, d_out, out_stride, stream=0):
    """n_frames RGB8 images of one size (image f at d_src + f * src_stride, any alignment) -> coded frames of the subword mode's geometry at
    d_out + f * out_stride: one compose launch, then the batch encoder; returns the coded word count of one frame."""
    n = C.c_uint64()
    _chk(lib().t3hip_encode_images_dev(C.c_void_p(d_src), C.c_int(sw), C.c_int(sh), C.c_uint64(src_stride), C.c_uint32(n_frames), C.c_int(int(sub)),
                                       C.c_int(1 if centered else 0), C.byref(cfg) if cfg is not None else None, C.c_void_p(d_out), C.c_uint64(out_stride), C.byref(n),
                                       C.c_void_p(stream)), "t3hip_encode_images_dev")
    return n.value

def interleave2d_dev(d_in, n, w, h, d_out, stream=0):
    """interleave2D_boustrophedon (OLD:750-813) of n device symbols into d_out (not d_in), asynchronous on `stream`."""
    _chk(lib().t3hip_interleave2d_dev(C.c_void_p(d_in), C.c_uint64(n), C.c_uint16(w), C.c_uint16(h), C.c_void_p(d_out), C.c_void_p(stream)), "t3hip_interleave2d_dev")


def rs_encode_blocks_dev(k, mode, d_data, n_blocks, d_code, stream=0):
    _chk(lib().t3hip_rs_encode_blocks_dev(C.c_int(k), C.c_int(mode), C.c_void_p(d_data), C.c_uint64(n_blocks), C.c_void_p(d_code), C.c_void_p(stream)), "t3hip_rs_encode_blocks_dev")


def rs_decode_blocks_dev(k, mode, d_code, n_blocks, d_data, d_ok, stream=0):
    _chk(lib().t3hip_rs_decode_blocks_dev(C.c_int(k), C.c_int(mode), C.c_void_p(d_code), C.c_uint64(n_blocks), C.c_void_p(d_data), C.c_void_p(d_ok), C.c_void_p(stream)), "t3hip_rs_decode_blocks_dev")


def inject_errors_dev(d_words, first_sym, n_blocks, seed, max_err, stream=0):
    _chk(lib().t3hip_inject_errors_dev(C.c_void_p(d_words), C.c_uint64(first_sym), C.c_uint64(n_blocks), C.c_uint32(seed), C.c_int(max_err), C.c_void_p(stream)), "t3hip_inject_errors_dev")


def frame_record_scratch_bytes(n_words=0):
    """Scratch t3hip_frame_record_dev wants (64 bytes still work: two accumulators, a fill kernel and atomics instead of per-workgroup partials)."""
    return int(lib().t3hip_frame_record_scratch_bytes(C.c_uint64(n_words)))


def frame_record_dev(d_words, n_words, frame_idx, cfg, d_rec, d_scratch, scratch_bytes=64, stream=0):
    _chk(lib().t3hip_frame_record_dev(C.c_void_p(d_words), C.c_uint64(n_words), C.c_uint64(frame_idx), C.byref(cfg), C.c_void_p(d_rec), C.c_void_p(d_scratch), C.c_uint64(scratch_bytes), C.c_void_p(stream)), "t3hip_frame_record_dev")


def crc32_dev(d_data, n_bytes, stream=0):
    """CRC-32 of a device buffer (the containers' payload CRC, io_t3p_t3v.cpp:20-36), computed by crc_chunks_kernel."""
    out = C.c_uint32()
    _chk(lib().t3hip_crc32_dev(C.c_void_p(d_data), C.c_uint64(n_bytes), C.byref(out), C.c_void_p(stream)), "t3hip_crc32_dev")
    return out.value


def crc32(data):
    """CRC-32 of host bytes: uploaded, then the same kernel (no CPU path)."""
    buf = _u8(data); out = C.c_uint32()
    _chk(lib().t3hip_crc32(_vp(buf), C.c_uint64(buf.size), C.byref(out)), "t3hip_crc32")
    return out.value


# ---- records and payload CRCs of N equal frames in one pass (include/t3hip.h) -------------------------------------------------
class RecordsPlan(C.Structure):
    """t3_records_plan: how frame_records_dev runs -- one pass (one CRC launch over all frames, one record launch) or a loop of the
    single-frame entry -- the CRC kernel and grid a frame gets, and the bytes and minimum stride of one frame."""
    _fields_ = [("n_frames", C.c_uint32), ("one_pass", C.c_uint8), ("form", C.c_uint8), ("pad_", C.c_uint8 * 2), ("stride_waves", C.c_uint32),
                ("wgs_per_frame", C.c_uint32), ("partials_per_frame", C.c_uint32), ("pad2_", C.c_uint32), ("frame_bytes", C.c_uint64),
                ("stride_min", C.c_uint64), ("scratch_bytes", C.c_uint64)]


RECORDS_TABLES, RECORDS_FP4 = 0, 1


def frame_records_scratch_bytes(n_words, n_frames):
    """Scratch frame_records_dev would like (16 * n_frames bytes still work: accumulators, one memset and atomics instead of partials)."""
    f = lib().t3hip_frame_records_scratch_bytes; f.restype = C.c_uint64     # (bound here, not in lib(): T3HIP_LIB may name an older build)
    return int(f(C.c_uint64(n_words), C.c_uint32(n_frames)))


def frame_records_plan(n_words, n_frames, n_cu=0, scratch_bytes=None):  # host only; n_cu = 0: the current context's device
    p = RecordsPlan()
    if scratch_bytes is None:
        scratch_bytes = frame_records_scratch_bytes(n_words, n_frames)
    _chk(lib().t3hip_frame_records_plan(C.c_uint64(n_words), C.c_uint32(n_frames), C.c_uint32(n_cu), C.c_uint64(scratch_bytes), C.byref(p)), "t3hip_frame_records_plan")
    return p


def frame_records_dev(d_words, n_words, stride, n_frames, first_idx, idx_step, cfg, d_recs, d_scratch, scratch_bytes, stream=0):
    """d_recs[f] = the record frame_record_dev writes for the frame at d_words + f * stride with frame_idx = first_idx + f * idx_step;
    asynchronous on `stream`.  Base, stride and scratch 16-byte aligned."""
    _chk(lib().t3hip_frame_records_dev(C.c_void_p(d_words), C.c_uint64(n_words), C.c_uint64(stride), C.c_uint32(n_frames), C.c_uint64(first_idx), C.c_uint64(idx_step),
                                       C.byref(cfg) if cfg is not None else None, C.c_void_p(d_recs), C.c_void_p(d_scratch), C.c_uint64(scratch_bytes), C.c_void_p(stream)),
         "t3hip_frame_records_dev")


def crc32_frames_dev(d_data, n_bytes, stride, n_frames, stream=0):
    """CRC-32 of n_frames device buffers of n_bytes at d_data + f * stride (16-byte aligned) in one pass; a list of n_frames ints."""
    out = (C.c_uint32 * max(n_frames, 1))()
    _chk(lib().t3hip_crc32_frames_dev(C.c_void_p(d_data), C.c_uint64(n_bytes), C.c_uint64(stride), C.c_uint32(n_frames), out, C.c_void_p(stream)), "t3hip_crc32_frames_dev")
    return [int(x) for x in out[:n_frames]]


def crc32_frames(frames):
    """CRC-32 of equally long host buffers, uploaded and done in one pass (no CPU path); ValueError for buffers of unequal size."""
    bufs = [_u8(f) for f in frames]
    if not bufs:
        return []
    if any(b.size != bufs[0].size for b in bufs):
        raise ValueError("crc32_frames: buffers of unequal size")
    ptrs = (C.c_void_p * len(bufs))(*[b.ctypes.data for b in bufs]); out = (C.c_uint32 * len(bufs))()
    _chk(lib().t3hip_crc32_frames(ptrs, C.c_uint64(bufs[0].size), C.c_uint32(len(bufs)), out), "t3hip_crc32_frames")
    return [int(x) for x in out]


def index_assemble(records_bytes, first_payload_offset=0):
    """records_bytes: uint8 array of concatenated t3_frame_record; returns a list of FrameRecord sorted by frame_idx with offsets."""
    buf = np.ascontiguousarray(records_bytes, np.uint8).copy()
    n = buf.size // FRAME_RECORD_BYTES
    _chk(lib().t3hip_index_assemble(_vp(buf), C.c_uint64(n), C.c_uint64(first_payload_offset)), "t3hip_index_assemble")
    return [FrameRecord.from_buffer_copy(buf[i * FRAME_RECORD_BYTES:(i + 1) * FRAME_RECORD_BYTES].tobytes()) for i in range(n)]


COMM_ID_BYTES = 128
PAD_FRAME_IDX = 2**64 - 1


def comm_available():
    """True when RCCL can be bound in this process (t3hip_comm_available: dlopen only -- no collective, no device call)."""
    return lib().t3hip_comm_available() == 0


def comm_unique_id():
    """Rank 0: the 128-byte rendezvous id of a new RCCL communicator (ncclGetUniqueId); hand it to the other ranks."""
    buf = (C.c_uint8 * COMM_ID_BYTES)()
    _chk(lib().t3hip_comm_unique_id(buf), "t3hip_comm_unique_id")
    return bytes(buf)


class Comm:
    """One RCCL communicator bound to this process's device (t3hip_comm_create after init()); the frame-index exchange
    step runs on it: index_allgather = ncclAllGather of 96-byte frame records, asynchronous on `stream`."""

    def __init__(self, unique_id, world, rank):
        self.h = C.c_void_p(); self.world, self.rank = world, rank
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(bytes(unique_id))
        _chk(lib().t3hip_comm_create(buf, C.c_int(world), C.c_int(rank), C.byref(self.h)), "t3hip_comm_create")

    def index_allgather(self, d_local, n_local, d_all, stream=0):
        _chk(lib().t3hip_index_allgather(self.h, C.c_void_p(d_local), C.c_uint64(n_local), C.c_void_p(d_all), C.c_void_p(stream)), "t3hip_index_allgather")

    def destroy(self):
        if self.h:
            lib().t3hip_comm_destroy(self.h); self.h = C.c_void_p()


class Event:
    """HIP event on the caller's stream (bench.py times kernels with these).  Timing only: created without the system-scope fence,
    it orders nothing and makes nothing visible (t3hip.h); read results after a stream or device synchronisation."""

    def __init__(self):
        self.h = C.c_void_p()
        _chk(lib().t3hip_event_create(C.byref(self.h)), "t3hip_event_create")

    def record(self, stream=0):
        _chk(lib().t3hip_event_record(self.h, C.c_void_p(stream)), "t3hip_event_record")

    def elapsed_ms(self, stop):
        ms = C.c_float()
        _chk(lib().t3hip_event_elapsed_ms(self.h, stop.h, C.byref(ms)), "t3hip_event_elapsed_ms")
        return ms.value

    def __del__(self):
        try:
            lib().t3hip_event_destroy(self.h)
        except Exception:
            pass
