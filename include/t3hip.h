/*
 * t3hip.h — C-ABI of libt3hip.so, the MI355X (gfx950) implementation of the
 * balanced-ternary Word27 encode/decode hot path.
 *
 * This is the drop-in boundary.  The reference has no FFI layer:
 * its path is header-only C++ over std::vector.  Each entry point below names
 * the reference function (file:line, OLD = old/include/ternary_image_codec_v6_min.hpp)
 * whose work it performs; include/ternary_codec_v6.hpp wraps these back into the
 * reference's own C++ names and signatures.
 *
 * Conventions
 *   - plain pointers + sizes, no C++/torch types; all structs are POD.
 *   - "words" are the reference's Word27 ABI: 9 bytes, one GF(27) symbol (0..26) each
 *     (OLD:666-669).  "pixels" are PixelYCbCrQuant: {u16 Yq; i16 Cbq; i16 Crq} = 6 bytes
 *     (OLD:670-674).
 *   - functions return T3_OK (0) or a negative T3_E_* code.  The reference's `bool`
 *     results map to: true = T3_OK, false = T3_E_HEADER / T3_E_RS / T3_E_ARG.
 *   - *_dev entry points take DEVICE pointers and a hipStream_t (as void*), never
 *     allocate caller-visible memory and never synchronise unless documented.
 *   - alignment of device buffers.  The profile ENCODE entry points (t3hip_encode_profile_dev, t3hip_encode_frame_dev, the coded
 *     output of t3hip_encode_rgb_dev / t3hip_encode_image_dev) want their buffers 16-byte aligned: T3_E_ARG otherwise, nothing
 *     written (RAW mode excepted; RGB input takes any alignment).  Consecutive frames packed into one buffer (9 * n_words bytes
 *     each) start on a 16-byte boundary only if the caller pads them.  The profile DECODE entry points (t3hip_decode_profile_dev,
 *     t3hip_decode_body_dev, t3hip_decode_frame_async, t3hip_decode_rgb_async; RAW mode excepted) take the coded stream and a
 *     pixel destination at any EVEN address -- an odd one is T3_E_ARG, nothing written -- and a raw-word or RGB destination at any
 *     address, and give the same bytes everywhere: 16-byte aligned buffers are the fast path, a coded stream elsewhere is read with
 *     unaligned accesses, a pixel destination elsewhere is written by the generic kernels, an RGB destination elsewhere through a
 *     pixel scratch and the bridge kernel.  The pack / unpack, subword, RGB-bridge, stage and CRC entry points take any alignment;
 *     the batch, window and image entry points state their own rule below.
 *   - a capacity argument (cap_words, cap_units, cap_px, cap_bytes, cap_trits, cap) is checked before anything is launched on the
 *     output: T3_E_CAPACITY leaves every byte of the output buffer -- and the verdict / failure words of the decode entry points --
 *     as it was, and the size the output needs, in the capacity's units, is stored through the call's size pointer (*n_out, *n_px,
 *     *n_words, *n_bytes, *n_trits).  t3hip_demap_rsdecode_bands_dev has no such pointer: t3hip_demap_rsdecode_bands_syms tells.
 *     This is about the call's own return code: t3hip_decode_frames can also meet a shortfall frame by frame (below).
 *     A capacity that is exactly that size is enough: no entry point writes a byte behind (or in front of) the units it returns.
 *   - there is no CPU fallback: compute entry points fail with T3_E_NODEVICE when
 *     no gfx950 device is usable.  Pure-metadata calls (plan, tables, header) are host-only.
 */
#ifndef T3HIP_H
#define T3HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes --------------------------------------------------------- */
#define T3_OK            0
#define T3_E_NODEVICE   -1  /* no usable HIP device / t3hip_init not successful   */
#define T3_E_HIP        -2  /* a HIP runtime call failed (see t3hip_last_hip_error) */
#define T3_E_ARG        -3  /* bad argument (null pointer, invalid subword, k ...) */
#define T3_E_CAPACITY   -4  /* caller's output buffer is too small                */
#define T3_E_HEADER     -5  /* header RS / CRC-12 failure  (OLD:920,929-934 -> false) */
#define T3_E_RS         -6  /* uncorrectable RS block      (OLD:987 -> false)     */
#define T3_E_COMM       -7  /* RCCL missing or a collective call failed (see t3hip_comm_last_error) */

/* ---- profile ids (OLD:34) -------------------------------------------------- */
#define T3_P1_RS26_24     0
#define T3_P2_RS26_22     1
#define T3_P3_RS26_20     2
#define T3_P4_RS26_18     3
#define T3_P5_RS26_22_2D  4
#define T3_RAW_MODE       0xFF

/* Arithmetic/framing flavour.
 * COMPAT: byte-exact with the reference (its non-RS "parity" map OLD:517-535, Forney
 *         with `add` OLD:658, its encoder/decoder framings as they are).
 * FIXED : true systematic RS consistent with the decoder's root convention, Forney
 *         with `sub`, self-consistent v6c framing so that
 *         decode(encode(x)) == x and <= t symbol errors per block are corrected.  A block is
 *         accepted only if register length = deg sigma = #roots <= t: ok <=> a codeword lies
 *         within t symbols of it (bounded distance), everything else is reported uncorrectable. */
#define T3_MODE_COMPAT 0
#define T3_MODE_FIXED  1

/* POD mirror of EncoderConfig (OLD:862-873) / DecoderConfigSeen (OLD:874-884). */
typedef struct t3_cfg {
    uint8_t  profile;            /* ProfileID value; T3_RAW_MODE = 0xFF          */
    uint8_t  band_profile[9];    /* UEPLayout::band_profile (OLD:60-63), used %4  */
    uint16_t tile_w, tile_h;     /* Tile2D (OLD:73-76)                            */
    uint32_t seed_a, seed_b, seed_s0;      /* ScramblerSeed (OLD:77-80)           */
    uint32_t beacon_words_period;          /* SparseBeaconCfg (OLD:95-100)        */
    uint8_t  beacon_band_slot;
    uint8_t  beacon_enabled;
    uint8_t  subword;            /* SubwordMode value 27/24/21/18/15 (OLD:117)    */
    uint8_t  centered;
    uint32_t superframe_words;   /* EncoderConfig::superframe_words (OLD:869)     */
    uint8_t  coset;              /* CosetID (OLD:114)                             */
    uint8_t  mode;               /* T3_MODE_COMPAT / T3_MODE_FIXED (build-side)   */
    uint8_t  reserved[2];
} t3_cfg;

/* Closed-form stream layout of one encode_profile_from_raw call (OLD:1043-1169). */
typedef struct t3_layout {
    uint64_t n_raw_words;        /* input Word27 count                            */
    uint64_t n_sym;              /* regrouped symbols = ceil(26*W/3)  (OLD:1051-1082) */
    uint64_t band_len[9];        /* symbols per band (i%9 split, OLD:1087-1088)   */
    uint64_t band_blocks[9];     /* RS blocks per band (tail dropped in COMPAT, OLD:1107) */
    uint64_t band_body_off[9];   /* first body symbol of each band (band-serial)  */
    uint64_t body_syms;          /* 26 * sum(band_blocks)                         */
    uint64_t body_syms_framed;   /* after beacon insertion (OLD:1118-1141)        */
    uint64_t out_syms;           /* header + framed body                          */
    uint64_t out_words;          /* ceil(out_syms/9) (OLD:1164)                   */
    uint32_t header_syms;        /* 52 in COMPAT (OLD:1159-1162), 90 in FIXED     */
    uint8_t  band_k[9];          /* RS k of each band (OLD:1089-1100)             */
    uint8_t  interleave2d;       /* 1 if P5 && tile.w && tile.h (OLD:1083)        */
    uint8_t  beacon_on;          /* 1 if beacon.enabled && period>0 (OLD:1118)    */
    uint8_t  pad_;
} t3_layout;

/* Fixed-size per-frame index record; the multi-GPU exchange step all-gathers these
 * (T3V frame index io_t3p_t3v.cpp:252-289). 96 bytes. */
typedef struct t3_frame_record {
    uint64_t frame_idx;
    uint64_t n_words;            /* coded Word27 count of the frame               */
    uint64_t byte_offset;        /* filled by t3hip_index_assemble (prefix sum)   */
    uint32_t crc32;              /* CRC-32 (poly 0xEDB88320) of the 9*n_words payload bytes */
    uint32_t sym_sum;            /* sum of all payload symbol bytes mod 2^32      */
    uint8_t  header_syms[54];    /* first 6 coded words (superframe header)       */
    uint8_t  profile;
    uint8_t  mode;
    uint8_t  pad_[8];
} t3_frame_record;

/* ---- lifecycle ---------------------------------------------------------------
 * A context = one GPU's stream, tables and scratch.  t3hip_init creates the process DEFAULT context on `device` (idempotent for
 * the same device; T3_E_ARG for another one while it exists: t3hip_shutdown first, or use t3hip_create).  A host that drives
 * several GPUs from one process -- the reference's language has no process-per-GPU launcher -- creates one context per device
 * (t3hip_create) and binds each of its worker threads to one with t3hip_use (thread-local; also makes that device current for
 * HIP).  Every entry point of this header works on the calling thread's context: the one given to t3hip_use, else the default.
 * Contexts are independent: two threads on two contexts never share a stream, a scratch buffer or a lock. */
typedef struct t3hip_ctx t3hip_ctx;
int         t3hip_device_count(void);
int         t3hip_init(int device);              /* the process default context           */
int         t3hip_shutdown(void);                /* destroys the default context          */
int         t3hip_is_ready(void);                /* 1 when the calling thread has a usable context */
int         t3hip_create(int device, t3hip_ctx** out);
int         t3hip_destroy(t3hip_ctx* ctx);       /* not the default context (that is t3hip_shutdown's) */
int         t3hip_use(t3hip_ctx* ctx);           /* bind the calling thread; NULL = back to the default */
t3hip_ctx*  t3hip_current(void);                 /* the calling thread's context (NULL if none)   */
int         t3hip_ctx_device(const t3hip_ctx* ctx);   /* its device index (-1 if none); NULL = current */
const char* t3hip_strerror(int code);
const char* t3hip_last_hip_error(void);
const char* t3hip_version(void);

/* ---- host-only metadata (no device needed) ------------------------------------ */
void t3hip_cfg_default(t3_cfg* cfg);                         /* EncoderContext() defaults OLD:862-873,898 */
int  t3hip_plan(uint64_t n_raw_words, const t3_cfg* cfg, t3_layout* out);
uint64_t t3hip_encoded_words(uint64_t n_raw_words, const t3_cfg* cfg);   /* 0 on bad cfg */
/* GF27Context::init tables (OLD:436-466): exp[78], log[27], mul[729], inv[27]. */
int  t3hip_gf27_tables(uint8_t* exp78, int16_t* log27, uint8_t* mul729, uint8_t* inv27);
/* RSCodec::build_gen (OLD:501-516): g[0..r], r = 26-k. */
int  t3hip_rs_generator(int k, uint8_t* g_out);
/* parity = data * P, P is k x (26-k) row-major (row i = parity of unit vector e_i). */
int  t3hip_rs_parity_matrix(int k, int mode, uint8_t* P_out);
/* Host only: the tables of the matrix-core encoder for one k, for inspection and CPU tests.
 * afrag[768]: A operand of v_mfma_i32_32x32x32_i8, 3 K-steps x 64 lanes x 4 dwords (trit coefficients as signed bytes);
 * lds_img[3168]: three 4-KiB scrambler-state tables (27 symbols x 32 bank copies: trits | scrambled symbol << 24), then
 * the three 128-byte mod-3 fold tables M_t[x] = 3^t ((x - 64) mod 3). */
int  t3hip_mfma_encode_tables(int k, int mode, uint32_t* afrag768, uint32_t* lds_img3168);
/* HeaderCodec::pack / check / unpack (OLD:206-380). */
int  t3hip_header_pack(const t3_cfg* cfg, uint32_t frame_seq, uint32_t band_map_hash, uint8_t syms27[27]);
int  t3hip_header_check(const uint8_t syms27[27]);           /* 1 ok, 0 bad */
int  t3hip_header_unpack(const uint8_t syms27[27], t3_cfg* out, uint32_t* frame_seq, uint32_t* band_map_hash);
/* The coded header symbols the encoder emits in front of the body (52 / 90). */
int  t3hip_header_encode(const t3_cfg* cfg, uint64_t n_raw_words, uint8_t* syms_out, uint32_t* n_syms);

/* ---- host-buffer entry points (what the std::vector API binds) ----------------- */
/* encode_raw_pixels_to_words OLD:723-734; words9 must hold (n_px+1)/2 words. */
int t3hip_pack_pixels(const void* px6, uint64_t n_px, void* words9);
/* decode_raw_words_to_pixels OLD:735-747; px6 must hold 2*n_words pixels. */
int t3hip_unpack_words(const void* words9, uint64_t n_words, void* px6);
/* encode_profile_from_raw OLD:1043-1169. */
int t3hip_encode_profile(const void* raw9, uint64_t n_raw, const t3_cfg* cfg,
                         void* out9, uint64_t cap_words, uint64_t* n_out);
/* decode_profile_to_raw OLD:995-1041.  `seen` is DecoderContext::cfg_last_seen: read for the
 * RAW shortcut, overwritten from the header once it decodes (OLD:1006-1013) — also when a
 * later RS block fails, as in the reference. */
int t3hip_decode_profile(const void* in9, uint64_t n_in, t3_cfg* seen,
                         void* out9, uint64_t cap_words, uint64_t* n_out);
/* Build-side conveniences named by the north star: pixels -> coded words in one fused
 * launch (= OLD:723 + OLD:1043), coded words -> pixels (= OLD:995 + OLD:735). */
int t3hip_encode_frame(const void* px6, uint64_t n_px, const t3_cfg* cfg,
                       void* out9, uint64_t cap_words, uint64_t* n_out);
int t3hip_decode_frame(const void* in9, uint64_t n_in, t3_cfg* seen,
                       void* px6, uint64_t cap_px, uint64_t* n_px);

/* ---- device-resident entry points (async on `stream` unless noted) ---------------- */
int t3hip_pack_pixels_dev(const void* d_px6, uint64_t n_px, void* d_words9, void* stream);
int t3hip_unpack_words_dev(const void* d_words9, uint64_t n_words, void* d_px6, void* stream);
int t3hip_encode_profile_dev(const void* d_raw9, uint64_t n_raw, const t3_cfg* cfg,
                             void* d_out9, uint64_t cap_words, uint64_t* n_out, void* stream);
int t3hip_encode_frame_dev(const void* d_px6, uint64_t n_px, const t3_cfg* cfg,
                           void* d_out9, uint64_t cap_words, uint64_t* n_out, void* stream);
/* Decode with the header parsed on the host: copies the 6 (COMPAT) / 10 (FIXED) header words
 * device->host and synchronises `stream` once, launches the body kernels, then synchronises
 * again to read the block-failure flag.  `to_pixels` selects Word27 or pixel output. */
int t3hip_decode_profile_dev(const void* d_in9, uint64_t n_in, t3_cfg* seen,
                             void* d_out, uint64_t cap_units, uint64_t* n_out,
                             int to_pixels, void* stream);
/* Fully asynchronous body decode for a caller that already knows the stream's config
 * (e.g. from t3hip_read_header_dev): no synchronisation; *d_fail (device u32) is
 * incremented for every uncorrectable block. */
int t3hip_read_header_dev(const void* d_in9, uint64_t n_in, int mode, t3_cfg* out_cfg,
                          uint64_t* n_raw_words, void* stream);            /* synchronises */
int t3hip_decode_body_dev(const void* d_in9, uint64_t n_in, const t3_cfg* cfg, uint64_t n_raw_words,
                          void* d_out, uint64_t cap_units, uint64_t* n_out, int to_pixels,
                          uint32_t* d_fail, void* stream);

/* Streaming decode, no synchronisation.  Frames of one stream repeat their configuration — the reference keeps it in
 * DecoderContext::cfg_last_seen (OLD:1006-1013) — so a caller that has parsed one frame's header (t3hip_decode_profile_dev
 * / t3hip_read_header_dev) decodes the following frames with that configuration: the body kernels are launched at once,
 * and a device-side check compares the frame's header symbols with the header `cfg` / `n_raw_words` encode to
 * (header RS + CRC-12, OLD:1142-1162).  Device words, zeroed and written by the call on `stream`:
 *   d_verdict[0] = 1 if the header differs (another configuration, or symbols that need the header's RS correction, or bytes above 26):
 *                  the output is then meaningless and the frame goes through t3hip_decode_profile_dev;
 *   d_verdict[1] = number of uncorrectable RS blocks (the reference's `false`, OLD:987).                          */
int t3hip_decode_frame_async(const void* d_in9, uint64_t n_in, const t3_cfg* cfg, uint64_t n_raw_words,
                             void* d_out, uint64_t cap_units, uint64_t* n_out, int to_pixels,
                             uint32_t* d_verdict, void* stream);

/* ---- the reference decoder's frame-sized stages, one at a time (OLD:938-993) ----------------------------------------
 * decode_profile_to_raw runs read_and_decode_header_from_words (stage 1, host: include/ternary_codec_v6.hpp), then these two on the
 * body behind the six header words.  t3hip_decode_profile* fuse them; these take them one by one.
 * descramble_words_inplace OLD:938-947: 9 * n_words bytes in place, any alignment; st = s0 % 3, then for every symbol in order
 *   st = (a * st + b) % 3 (uint32 wrap-around) and st is subtracted from each trit.  Asynchronous.
 * demap_and_rsdecode_bands_from_words OLD:948-993 on a DESCRAMBLED body: band b = slot b of every word, except the words
 *   wi % beacon_words_period == 0 in band beacon_band_slot when beacon_enabled && beacon_words_period > 0 (a slot >= 9 never matches,
 *   a period of 1 empties that band); band b is decoded with code q = band_profile[b] % 4, i.e. RS(26, code_k[q]) in arithmetic
 *   code_mode[q] (T3_MODE_*), whole blocks of 26 only.  Output: the k data symbols of every block, band-major.  Only hdr's
 *   band_profile and beacon_* fields are read; every field is taken as it is (none reduced).  A code a band uses with k outside
 *   {18, 20, 22, 24} or a mode above 1 is T3_E_ARG.
 *   _syms: the output size (0 on bad arguments).
 *   _dev:  no synchronisation.  *d_n_valid (device, 8-byte aligned) is set to the output size and lowered to the output offset of
 *          every block whose decode_block is false: afterwards it is the length of the prefix the reference leaves in out_syms when
 *          it returns false at its first failing block (= the size when every block decoded).  Bytes from *d_n_valid on are unspecified.
 *   host:  T3_OK (*n_out = size), T3_E_RS (*n_out = the valid prefix, out holds it), T3_E_ARG, T3_E_CAPACITY (*n_out = size). */
int t3hip_descramble_words_dev(void* d_words9, uint64_t n_words, uint32_t a, uint32_t b, uint32_t s0, void* stream);
int t3hip_descramble_words(void* words9, uint64_t n_words, uint32_t a, uint32_t b, uint32_t s0);
uint64_t t3hip_demap_rsdecode_bands_syms(uint64_t n_words, const t3_cfg* hdr, const uint8_t code_k[4]);
int t3hip_demap_rsdecode_bands_dev(const void* d_body9, uint64_t n_words, const t3_cfg* hdr, const uint8_t code_k[4], const uint8_t code_mode[4],
                                   uint8_t* d_out, uint64_t cap, uint64_t* d_n_valid, void* stream);
int t3hip_demap_rsdecode_bands(const void* body9, uint64_t n_words, const t3_cfg* hdr, const uint8_t code_k[4], const uint8_t code_mode[4],
                               uint8_t* out, uint64_t cap, uint64_t* n_out);

/* ---- block-level RS(26,k) (RSCodec::encode_block OLD:517-535, decode_block OLD:546-662) */
int t3hip_rs_encode_blocks_dev(int k, int mode, const uint8_t* d_data_k, uint64_t n_blocks,
                               uint8_t* d_code26, void* stream);
/* Block-level symbols above 26 are outside the contract: the reference indexes past its tables with them, so no behaviour exists to match.
 * d_code26 is corrected in place (inout_n), d_data_k receives the first k symbols (out_k),
 * d_ok[b] = 1/0 is decode_block's return value.  On a 0 the reference leaves inout_n
 * partially modified and out_k untouched; so does this. */
int t3hip_rs_decode_blocks_dev(int k, int mode, uint8_t* d_code26, uint64_t n_blocks,
                               uint8_t* d_data_k, uint8_t* d_ok, void* stream);

/* Host-buffer forms (what RSCodec::encode_block / decode_block of include/ternary_codec_v6.hpp bind): upload, the kernels above,
 * download.  data_k of a block whose decode fails is returned as it came in (the reference leaves out_k untouched). */
int t3hip_rs_encode_blocks(int k, int mode, const uint8_t* data_k, uint64_t n_blocks, uint8_t* code26);
int t3hip_rs_decode_blocks(int k, int mode, uint8_t* code26_inout, uint64_t n_blocks, uint8_t* data_k, uint8_t* ok);
/* ONE block, on the host (no device, no launch): what RSCodec::encode_block / decode_block bind when a caller walks blocks one at a
 * time (the reference's self-test OLD:1172-1207, its header RS OLD:1142-1158).  26 bytes are control data, like the header codec;
 * same parity matrix / decoder as the kernels.  decode returns 1 (decode_block true), 0 (false; out_k untouched) or T3_E_ARG. */
int t3hip_rs_encode_block_host(int k, int mode, const uint8_t* data_k, uint8_t* code26);
int t3hip_rs_decode_block_host(int k, int mode, uint8_t* code26_inout, uint8_t* data_k);

/* ---- the reference's symbol-level public helpers --------------------------------------------------------
 * Single symbols and the header are control data: host arithmetic on the tables the kernels are built from.
 *   gf27_add / gf27_sub / gf27_mul_poly OLD:383-413 (operands reduced mod 27)
 *   scramble_symbol / descramble_symbol OLD:81-94: *st <- (a * *st + b) % 3 in uint32 wrap-around, then every trit of s +/- *st
 *   encode_beacon_symbol OLD:107-113;  CRC3::rem12 OLD:176-205 (ternary CRC-12 of n trits, 12 zero trits appended)
 * interleave2D_boustrophedon / deinterleave2D_boustrophedon OLD:750-813 on a symbol vector: device kernel (the map is an
 * involution inside every row segment, so `inverse` selects nothing); w == 0 or h == 0 leaves the symbols as they are. */
uint8_t t3hip_gf27_add(uint8_t a, uint8_t b);
uint8_t t3hip_gf27_sub(uint8_t a, uint8_t b);
uint8_t t3hip_gf27_mul(uint8_t a, uint8_t b);
uint8_t t3hip_scramble_symbol(uint8_t s, uint32_t a, uint32_t b, uint32_t* st, int inverse);
uint8_t t3hip_beacon_symbol(uint8_t profile, uint16_t frame_seq_mod, uint8_t health_flags);
int t3hip_crc12(const uint8_t* trits, uint64_t n, uint8_t out12[12]);
int t3hip_interleave2d(uint8_t* syms, uint64_t n, uint16_t w, uint16_t h, int inverse);
int t3hip_interleave2d_dev(const uint8_t* d_in, uint64_t n, uint16_t w, uint16_t h, uint8_t* d_out, void* stream);   /* d_out != d_in */

/* ---- trit error injector for the recovery test ------------------ */
/* For every 26-symbol block of the body region [first_sym, first_sym+26*n_blocks): a counter hash of
 * (seed, block) picks e in 0..max_err distinct positions and alters one trit of each. */
int t3hip_inject_errors_dev(void* d_words9, uint64_t first_sym, uint64_t n_blocks,
                            uint32_t seed, int max_err, void* stream);

/* ---- frame index record (multi-GPU exchange payload) -------------------------------- */
/* d_scratch: device memory the call may use until the record is written (stream-ordered), 4-byte aligned, content irrelevant.
 * t3hip_frame_record_scratch_bytes() says how much it would like (one partial result per CRC workgroup: no zeroing pass, no atomics);
 * anything from 8 bytes up works (two accumulators, zeroed by a fill in front of the CRC kernel). */
int t3hip_frame_record_dev(const void* d_words9, uint64_t n_words, uint64_t frame_idx,
                           const t3_cfg* cfg, t3_frame_record* d_rec, void* d_scratch,
                           uint64_t scratch_bytes, void* stream);
uint64_t t3hip_frame_record_scratch_bytes(uint64_t n_words);
/* Payload CRC of the T3P6/T3V6 containers (crc32_acc, src/io_t3p_t3v.cpp:20-36: poly 0xEDB88320, init and final
 * inversion 0xFFFFFFFF) of a device buffer / a host buffer (uploaded, same kernel).  Synchronous: *crc_out is host
 * memory and valid on return.  n_bytes == 0 gives 0, which is also what the containers store for an empty payload. */
int t3hip_crc32_dev(const void* d_data, uint64_t n_bytes, uint32_t* crc_out, void* stream);
int t3hip_crc32(const void* data, uint64_t n_bytes, uint32_t* crc_out);
/* The records, or the payload CRCs, of N equal frames in one pass: frame f's n_words coded words start f * stride bytes behind frame 0's
 * (what t3hip_encode_frames_dev leaves), and d_recs[f] is, byte for byte, the record t3hip_frame_record_dev writes for frame f alone with
 * frame_idx = first_idx + f * idx_step (a rank's local frames are rank, rank + world, ...: first_idx = rank, idx_step = world).
 *   one pass   at most one memset, ONE CRC launch over (workgroups per frame) x n_frames and ONE record launch, where the single-frame
 *              entry costs each frame a memset, a CRC launch and a record launch: a small frame gets a fraction of the part's wave slots
 *              (t3_records_plan.stride_waves of 8 per CU), and N of them fill it together.  Every frame is planned as the single-frame
 *              entry plans one such frame.  One frame, the T3HIP_CRC_BLOCKED measurement knob and streams of 2^40 bytes or more are a loop
 *              of the single-frame entry inside the call (one_pass = 0): same bytes out.
 *   alignment  the rule of the batch entries below: base 16-byte aligned, stride a multiple of 16 and at least stride_min = 9 * n_words rounded up to
 *              16, no null base where there are words, n_frames <= 65535; T3_E_ARG otherwise, before the call asks for a device.
 *   scratch    (t3hip_frame_records_dev) device memory the call may use until the records are written, 16-BYTE ALIGNED, content
 *              irrelevant, cut into n_frames slots of (scratch_bytes / n_frames) & ~15 bytes.  t3hip_frame_records_scratch_bytes() is
 *              what it would like (a slot then holds one partial result per CRC workgroup: no memset, no atomics); any size from
 *              16 * n_frames up works (two accumulators per slot, zeroed by the one memset).  The decision is the same for every frame.
 *   n_frames   0: T3_OK, nothing touched.  n_words == 0: no CRC launch, records with crc32 == 0, as the single-frame entry writes them.
 * t3hip_frame_records_plan is host only: n_cu = 0 plans for the current context's device (T3_E_NODEVICE without one), an explicit n_cu
 * needs no device.  t3hip_frame_records_dev is asynchronous on `stream`.
 * t3hip_crc32_frames_dev / t3hip_crc32_frames: the containers' payload CRC (t3hip_crc32[_dev]) of N equal buffers of n_bytes -- device
 * buffers at `stride` (the same alignment rule, with stride_min = n_bytes rounded up to 16), or host buffers by pointer, uploaded at a
 * 16-byte stride -- with ONE pass on the context's own scratch, one copy back and one synchronisation where N calls of t3hip_crc32[_dev]
 * drain the stream N times.  Synchronous: crc_out[n_frames] is host memory and valid on return; n_bytes == 0 gives zeros. */
#define T3_RECORDS_TABLES 0          /* t3_records_plan.form: the table kernel (frames below 64 rounds of 2 KiB, T3HIP_CRC_TABLES)  */
#define T3_RECORDS_FP4    1          /*                       the matrix-core kernel, strided rounds                               */
typedef struct t3_records_plan {
    uint32_t n_frames;
    uint8_t  one_pass;               /* 1: the one pass above; 0: a loop of the single-frame entry                                 */
    uint8_t  form;                   /* T3_RECORDS_* : the CRC kernel a frame gets                                                 */
    uint8_t  pad_[2];
    uint32_t stride_waves;           /* FP4: the waves W a frame's rounds are strided over (wave g: rounds g, g + W, ...); else 0  */
    uint32_t wgs_per_frame;          /* CRC workgroups per frame: W / 4, one more when 9 * n_words is no multiple of 2048          */
    uint32_t partials_per_frame;     /* = wgs_per_frame when a slot has room for them (64 + 8 * wgs_per_frame bytes), else 0       */
    uint32_t pad2_;
    uint64_t frame_bytes, stride_min;/* 9 * n_words; that, rounded up to 16                                                        */
    uint64_t scratch_bytes;          /* n_frames * slot bytes: the part of the caller's scratch the pass uses                      */
} t3_records_plan;
int t3hip_frame_records_plan(uint64_t n_words, uint32_t n_frames, uint32_t n_cu, uint64_t scratch_bytes, t3_records_plan* out);
uint64_t t3hip_frame_records_scratch_bytes(uint64_t n_words, uint32_t n_frames);
int t3hip_frame_records_dev(const void* d_words9, uint64_t n_words, uint64_t stride, uint32_t n_frames, uint64_t first_idx, uint64_t idx_step,
                            const t3_cfg* cfg, t3_frame_record* d_recs, void* d_scratch, uint64_t scratch_bytes, void* stream);
int t3hip_crc32_frames_dev(const void* d_data, uint64_t n_bytes, uint64_t stride, uint32_t n_frames, uint32_t* crc_out, void* stream);
int t3hip_crc32_frames(const void* const* frames, uint64_t n_bytes, uint32_t n_frames, uint32_t* crc_out);
/* Host: sort gathered records by frame_idx and fill byte_offset (T3V index, io_t3p_t3v.cpp:252-289). */
int t3hip_index_assemble(t3_frame_record* recs, uint64_t n_recs, uint64_t first_payload_offset);

/* ---- multi-GPU exchange step ------------------------------------------------------
 * Frames shard round-robin over GPUs with no data-path collective; the only exchange is one all-gather of the fixed-size
 * frame records above, from which every rank assembles the T3V frame index (io_t3p_t3v.cpp:252-289: offset, words per
 * frame) with t3hip_index_assemble.  The reference has no collective at all; a C++ host does
 *   rank 0: t3hip_comm_unique_id(id) -> hands the 128 bytes to the other ranks by its own means (file, socket, MPI, ...)
 *   every rank, after t3hip_init(device): t3hip_comm_create(id, world, rank, &c)         (ncclCommInitRank)
 *   per batch: t3hip_index_allgather(c, d_local, n_local, d_all, stream)                  (ncclAllGather, asynchronous)
 * RCCL is bound at run time (dlopen librccl.so.1); without it these return T3_E_COMM. */
#define T3_COMM_ID_BYTES 128
typedef struct t3_comm t3_comm;
/* T3_OK when RCCL can be bound in this process, T3_E_COMM otherwise; no collective, no device call.  A multi-rank host probes this on
 * EVERY rank and agrees on the result (its own control channel) before anyone draws an id or calls t3hip_comm_create: a rank that
 * cannot bind must not leave the others waiting inside ncclCommInitRank. */
int t3hip_comm_available(void);
int t3hip_comm_unique_id(uint8_t id[T3_COMM_ID_BYTES]);
int t3hip_comm_create(const uint8_t id[T3_COMM_ID_BYTES], int world, int rank, t3_comm** out);
int t3hip_comm_destroy(t3_comm* c);
int t3hip_comm_world(const t3_comm* c);
int t3hip_comm_rank(const t3_comm* c);
const char* t3hip_comm_last_error(void);
/* d_local: n_local records of this rank (device); d_all: world * n_local records (device), rank-major.  Every rank passes the
 * same n_local (pad with records whose frame_idx == UINT64_MAX). */
int t3hip_index_allgather(t3_comm* c, const t3_frame_record* d_local, uint64_t n_local, t3_frame_record* d_all, void* stream);

/* ---- subword trit streams and wire packings ------------------------------
 * One byte per trit (0..2) on the trit side.  N = trits kept per word (SubwordMode: 27/24/21/18/15; any 1..27 accepted).
 *   extract : extract_subword_stream_from_words  OLD:834-844 -> n_words * N trits (first N trits of every word)
 *   build   : build_words_from_subword_stream    OLD:845-859 -> ceil(n_trits / N) words; slots N..26 = fill, a short last
 *             group is zero-padded up to N
 *   base243 : tpack::ut_to_base243 / base243_to_ut  TPACK:28-50: uint32 LE trit count, then 5 trits per byte (LSD first);
 *             unpack returns T3_E_HEADER where the reference returns false (short input, fewer trits than announced)
 *   mod27   : tpack::words_to_bytes / bytes_to_words  TPACK:53-65: every byte % 27 (callers check n % 9 for bytes_to_words) */
uint64_t t3hip_subword_words(uint64_t n_trits, int N);
uint64_t t3hip_base243_bytes(uint64_t n_trits);
int t3hip_subword_extract(const void* words9, uint64_t n_words, int N, uint8_t* trits);
int t3hip_subword_build(const uint8_t* trits, uint64_t n_trits, int N, uint8_t fill, void* words9, uint64_t cap_words, uint64_t* n_words);
int t3hip_base243_pack(const uint8_t* trits, uint64_t n_trits, uint8_t* out, uint64_t cap_bytes, uint64_t* n_bytes);
int t3hip_base243_unpack(const uint8_t* in, uint64_t n_bytes, uint8_t* trits, uint64_t cap_trits, uint64_t* n_trits);
int t3hip_mod27_bytes(const uint8_t* in, uint64_t n, uint8_t* out);
int t3hip_subword_extract_dev(const void* d_words9, uint64_t n_words, int N, uint8_t* d_trits, void* stream);
int t3hip_subword_build_dev(const uint8_t* d_trits, uint64_t n_trits, int N, uint8_t fill, void* d_words9, uint64_t cap_words, uint64_t* n_words, void* stream);
int t3hip_base243_pack_dev(const uint8_t* d_trits, uint64_t n_trits, uint8_t* d_out, uint64_t cap_bytes, uint64_t* n_bytes, void* stream);
/* total = the trit count of the 4-byte header (the host entry point reads it itself) */
int t3hip_base243_unpack_dev(const uint8_t* d_in, uint64_t n_bytes, uint64_t total, uint8_t* d_trits, void* stream);
int t3hip_mod27_bytes_dev(const uint8_t* d_in, uint64_t n, uint8_t* d_out, void* stream);
/* Centring blits of row f3, old/include/io_image.hpp:125-140 (blit_center_rgb) and :215-235 (extract_center_q); parity unpinned
 * like the rest of io_image.hpp (restated from the text, checked against the oracle's restatement).
 *   blit    : sw x sh RGB8 image into the middle of a zeroed cw x ch canvas, x0 = max(0,(cw-sw)/2), y0 = max(0,(ch-sh)/2); source
 *             rows that fall below the canvas are dropped.  sw > cw is T3_E_ARG (the reference overruns the canvas row there).
 *   extract : the sw x sh window in the middle of a fw x fh frame of 6-byte pixels; window rows below the frame come out zero.
 *             sw > fw is T3_E_ARG (the reference reads on into the next frame row).
 * Device pointers: destination 4-byte aligned. */
int t3hip_blit_center_rgb(const uint8_t* src, int sw, int sh, uint8_t* dst, int cw, int ch);
int t3hip_extract_center_q(const void* full_px6, int fw, int fh, void* sub_px6, int sw, int sh);
int t3hip_blit_center_rgb_dev(const uint8_t* d_src, int sw, int sh, uint8_t* d_dst, int cw, int ch, void* stream);
int t3hip_extract_center_q_dev(const void* d_full_px6, int fw, int fh, void* d_sub_px6, int sw, int sh, void* stream);

/* ---- SURVEY 8 row f1 (first version, own kernels): RGB8 <-> quantised YCbCr bridge ------------
 * rgb_to_quant_stream / quant_stream_to_rgb, old/include/io_image.hpp:47-90,156-195: float BT.601-style conversion with
 * std::lround and clamps, then quantisation in double.  rgb = 3 bytes per pixel (R,G,B), px6 = PixelYCbCrQuant[n_px].
 * Bit-exact against the oracle's restatement for all 2^24 RGB values; parity UNPINNED against a reference build (that
 * header does not compile: ImageU8::swap, old/include/io_image.hpp:218). */
int t3hip_rgb_to_quant(const uint8_t* rgb, uint64_t n_px, void* px6);
int t3hip_quant_to_rgb(const void* px6, uint64_t n_px, uint8_t* rgb);
int t3hip_rgb_to_quant_dev(const uint8_t* d_rgb, uint64_t n_px, void* d_px6, void* stream);
int t3hip_quant_to_rgb_dev(const void* d_px6, uint64_t n_px, uint8_t* d_rgb, void* stream);
/* RGB frame -> coded stream and back in one call each (what a caller of io_image.hpp's rgb_to_quant_stream +
 * encode_raw_pixels_to_words + encode_profile_from_raw does, old/src/main.cpp:12-19): the bridge kernel into a per-stream
 * scratch, then the fused encode / after the decode.  Both asynchronous on `stream`; the decode uses the streaming entry
 * (known configuration, d_verdict as for t3hip_decode_frame_async).  n_px pixels -> (n_px + 1) / 2 raw words. */
int t3hip_encode_rgb_dev(const uint8_t* d_rgb, uint64_t n_px, const t3_cfg* cfg, void* d_out9, uint64_t cap_words,
                         uint64_t* n_out, void* stream);
int t3hip_decode_rgb_async(const void* d_in9, uint64_t n_in, const t3_cfg* cfg, uint64_t n_px, uint8_t* d_rgb,
                           uint32_t* d_verdict, void* stream);

/* ---- window decode: a pixel window of a coded frame from the tiles it covers -------------------------------------------
 * The frame's decoded pixel stream -- the 2 * n_raw_words pixels t3hip_decode_frame_async(..., to_pixels = 1) returns -- is read as
 * rows of fw pixels; output pixel (x, y), 0 <= x < w, 0 <= y < h, is stream pixel (y0 + y) * fw + x0 + x.  A position in a row >= fh
 * or behind the end of the stream is a zero pixel record, in RGB (0, 0, 0): what extract_center_q followed by quant_stream_to_rgb
 * give (old/include/io_image.hpp:215-235, :184-206).  fw * fh need not equal the pixel count.  x0 + w > fw, fw == 0, RAW mode:
 * T3_E_ARG.  w * h == 0: T3_OK, nothing launched, d_verdict untouched.
 * Two paths, chosen by t3hip_window_plan (host only, launches nothing):
 *   tile range   FIXED, one k on all bands, 1-D, no beacon: such a stream is made of independent pixel tiles (108 * k pixels each); only
 *                the tiles [tile_lo, tile_hi) that hold stream pixels (y0 * fw + x0) .. ((y0 + h - 1) * fw + x0 + w) are decoded --
 *                only their band runs are read -- into a per-stream scratch sized for that run, and the window is cut from it.
 *   whole frame  every other framing t3hip_decode_frame_async accepts (per-band k, 2-D, beacon, COMPAT): the frame is decoded into the
 *                scratch, then the same cut; what that entry refuses, this one refuses with the same code.  Slower, same bytes out.
 * d_verdict[0] is the header verdict of t3hip_decode_frame_async.  d_verdict[1] counts the uncorrectable blocks AMONG THE BLOCKS THAT
 * WERE DECODED, which always include every block a window pixel comes from: on the tile-range path a bad block in a tile the window
 * does not touch does not spoil the window (and is not reported) -- a viewer or cropper pays for, and depends on, its own tiles only.
 * Asynchronous, no synchronisation.  d_in9 as for t3hip_decode_frame_async; d_out 4-byte aligned.
 * out_fmt 1 = PixelYCbCrQuant (6 bytes), 2 = RGB8 (3 bytes; bit-identical to t3hip_quant_to_rgb_dev on the window's pixels). */
typedef struct t3_window_plan {
    uint32_t n_tiles;            /* pixel tiles of the whole frame on the path chosen (0 on the whole-frame path) */
    uint32_t tile_lo, tile_hi;   /* tiles launched: [tile_lo, tile_hi); equal when no window pixel is in the stream */
    uint64_t first_px, n_px;     /* the run of stream pixels those tiles produce                                   */
    uint8_t  tile_range;         /* 1: only that range is decoded; 0: the whole frame is decoded, then cropped     */
    uint8_t  pad_[7];
} t3_window_plan;
int t3hip_window_plan(uint64_t n_raw_words, const t3_cfg* cfg, uint32_t fw, uint32_t fh,
                      uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, t3_window_plan* out);
int t3hip_decode_window_async(const void* d_in9, uint64_t n_in, const t3_cfg* cfg, uint64_t n_raw_words,
                              uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                              void* d_out, int out_fmt, uint32_t* d_verdict, void* stream);

/* ---- batches of equal frames: N frames of one configuration and one size in one call (video, old/src/main_video_t3v.cpp:24-26) ----
 * Frame f of a batch starts f * stride bytes behind frame 0, in the input and in the output; all frames share `cfg` and the unit count,
 * so one t3_layout and one coded header serve them all (frame_seq is never written, OLD:1142-1150).  fmt names the unit side of the call:
 * 0 raw Word27 (9 bytes), 1 PixelYCbCrQuant (6 bytes), 2 RGB8 (3 bytes).  n_units pixels make (n_units + 1) / 2 raw words; a decode
 * writes 2 * n_raw_words pixels (fmt 1, 2: an odd frame's pad pixel included) or n_raw_words words (fmt 0).
 *   alignment  bases 16-byte aligned, strides multiples of 16 and at least the plan's *_stride_min (the rule of this header's device
 *              entry points, padded as it tells callers to); anything else: T3_E_ARG.  Bytes of a stride behind a frame's own bytes
 *              are never written.  A null base of a batch that has bytes to read or write is T3_E_ARG as well; the _dev / _async
 *              entries refuse all of this before they ask for a device (T3_E_NODEVICE comes after the argument checks).
 *   one_launch a batch whose plan says one_launch = 1 runs as that one launch or is refused (T3_E_ARG); it never takes the loop.
 *   verdicts   d_verdict[2 f], d_verdict[2 f + 1]: the two words of t3hip_decode_frame_async for frame f alone.  A damaged frame
 *              touches neither its neighbours' words nor their pixels.
 *   n_frames   0: T3_OK, nothing launched.  1: the single-frame entry.  More than 65535, or n_frames * tiles_per_frame >= 2^31 on
 *              the one-launch path: T3_E_ARG.
 *   one launch (one_launch = 1: ONE codec kernel over the tile space of all frames, so the launch's fixed cost -- tables into LDS,
 *              the ticket drain -- is paid once and small frames fill the part together) exactly where the fused single-k kernels serve a
 *              frame: encode -- pixel or RGB input, one k on all bands, 1-D, no beacon, COMPAT and FIXED; decode -- FIXED, one k, 1-D, no
 *              beacon, pixel or RGB output; both with n_raw_words > 0 and n_frames >= 2.
 *   per frame  (one_launch = 0) everything else the single-frame entries accept -- raw words either way, per-band k, 2-D, beacon, COMPAT
 *              decode, RAW mode -- is a loop of those entries inside the call: same bytes out, same verdict words; what they refuse, the
 *              batch refuses with the same code.
 * t3hip_frames_plan is host only and launches nothing.  The _dev / _async entries are asynchronous on `stream`; two batched calls back
 * to back on one stream need nothing in between.  The host entries take host buffers with the same strides as on the device: one
 * upload, the device entry, one download.  t3hip_decode_frames reads frame 0's header as t3hip_decode_profile does (T3_E_HEADER if it
 * does not decode), decodes the batch with that configuration, sends every frame whose header verdict is 1 through the single-frame path
 * on its own, fills frame_rc[f] (T3_OK / T3_E_HEADER / T3_E_RS; T3_E_CAPACITY for a frame of a COMPAT or RAW-mode batch -- whose size only
 * its own header tells -- that has more than cap_units units: the call still returns T3_OK) and writes `seen` as the single-frame entry would for frame 0; it
 * returns T3_OK when the call itself went through, whatever the frames' own codes; seen->mode selects the flavour on entry, as there, and
 * cap_units * unit bytes <= out_stride.  Streams the batch entry does not plan from a header (COMPAT, RAW mode) go frame by frame through
 * t3hip_decode_profile_dev.  n_in / n_out_words: coded words of ONE frame. */
typedef struct t3_frames_plan {
    uint32_t n_frames, tiles_per_frame;      /* tiles_per_frame = 0 on the per-frame path                          */
    uint8_t  one_launch;                     /* 1: all frames in one codec launch; 0: a loop of the single-frame path */
    uint8_t  pad_[7];
    uint64_t in_bytes, out_bytes;            /* bytes one frame reads / writes                                     */
    uint64_t in_stride_min, out_stride_min;  /* those, rounded up to 16                                            */
} t3_frames_plan;
int t3hip_frames_plan(int decode, uint64_t n_units, uint32_t n_frames, const t3_cfg* cfg, int fmt, t3_frames_plan* out);
int t3hip_encode_frames_dev(const void* d_in, uint64_t n_units, int in_fmt, uint64_t in_stride, uint32_t n_frames, const t3_cfg* cfg,
                            void* d_out9, uint64_t out_stride, uint64_t* n_out_words, void* stream);
int t3hip_decode_frames_async(const void* d_in9, uint64_t n_in, uint64_t in_stride, uint32_t n_frames, const t3_cfg* cfg,
                              uint64_t n_raw_words, void* d_out, uint64_t out_stride, int out_fmt,
                              uint32_t* d_verdict /* 2 * n_frames words */, void* stream);
int t3hip_encode_frames(const void* in, uint64_t n_units, int in_fmt, uint64_t in_stride, uint32_t n_frames, const t3_cfg* cfg,
                        void* out9, uint64_t out_stride, uint64_t* n_out_words);
int t3hip_decode_frames(const void* in9, uint64_t n_in, uint64_t in_stride, uint32_t n_frames,
                        void* out, uint64_t out_stride, uint64_t cap_units /* per frame */, int out_fmt,
                        t3_cfg* seen, uint64_t* n_out /* units of one frame */, int* frame_rc /* n_frames */);

/* The same window out of every frame of a batch (a video cropper or viewer): t3hip_decode_window_async over N equal frames in one call.
 * Frame f's window -- the window definition, the zero pixels past fh or behind the stream, out_fmt 1 / 2 are those of the window
 * entry -- is written at d_out + f * out_stride, byte for byte what t3hip_decode_window_async writes for frame f alone, and
 * d_verdict[2 f], d_verdict[2 f + 1] are that entry's two words for frame f alone.  A damaged frame touches neither its neighbours'
 * words nor their pixels, and an uncorrectable block in a tile the window does not cover is neither decoded nor reported.
 *   alignment  the batch rule above, against this plan's in_stride_min (coded bytes of a frame) and out_stride_min (w * h * (6 | 3));
 *              a null base of a batch with bytes to move, a missing verdict pointer: T3_E_ARG.  Every argument refusal comes before
 *              the call asks for a device; T3_E_NODEVICE comes last.
 *   n_frames   0: T3_OK, nothing launched.  1: the single-frame entry.  More than 65535 (the crop's grid), or
 *              n_frames * (tile_hi - tile_lo) >= 2^31 on the one-launch path: T3_E_ARG.
 *   w * h == 0 T3_OK, nothing launched, verdicts untouched.  RAW mode, x0 + w > fw, fw == 0, out_fmt other than 1 / 2: T3_E_ARG.
 *   one launch (one_launch = 1) where the frame's own window plan says tile_range = 1 (FIXED, one k, 1-D, no beacon), tile_hi > tile_lo
 *              and n_frames >= 2: one hipMemsetAsync of the verdict words, ONE launch of the fused pixel decoder over
 *              n_frames * (tile_hi - tile_lo) tile tickets -- every frame's tile range into a per-stream scratch, frame f's run at
 *              f * r16(6 * win.n_px) -- and ONE crop launch over the runs.  A plan that says one launch runs as one launch or is
 *              refused (T3_E_ARG); it never silently takes the loop.  A truncated stream (fewer than the plan's coded words in n_in) is
 *              T3_E_HEADER, as in the single-frame entry.  (The plan is not told n_in: a call with 9 * n_in >= 2^32 is the loop below.)
 *   per frame  (one_launch = 0) everything else -- per-band k, 2-D, beacon and COMPAT frames, a window wholly behind the stream, one frame
 *              -- is a loop of t3hip_decode_window_async inside the call: the same bytes, the same words, the same refusals with the
 *              same codes.
 *   scratch_bytes  the per-stream scratch the call holds: n_frames * r16(6 * win.n_px) + 256 on the one-launch path (the 256 are the
 *              single-frame entry's slack behind the run), that entry's own scratch on the loop path, 0 when nothing is launched.
 * t3hip_frames_window_plan is host only and launches nothing.  t3hip_decode_frames_window takes host buffers with the device strides:
 * one upload, the device entry, one synchronisation, one download.  frame_rc[f] is T3_OK, T3_E_RS or T3_E_HEADER: a frame whose header
 * verdict is 1 goes through t3hip_read_header_dev on its own; if that header decodes to the caller's configuration and word count the
 * frame is redone by the single-frame window entry (and its block count decides), else it is T3_E_HEADER.  The call returns T3_OK when
 * the call itself went through, whatever the frames' own codes.
 * t3hip_decode_images_async is this entry on t3hip_image_geometry(sub, centered): n_raw_words = fw * fh / 2, the window is the target
 * rectangle, RGB out (out_stride >= r16(tw * th * 3)) -- for a batch what t3hip_decode_image_async is for one frame. */
typedef struct t3_frames_window_plan {
    t3_window_plan win;                       /* the plan of ONE frame; every frame of the batch shares it        */
    uint32_t n_frames;
    uint8_t  one_launch;                      /* 1: one decoder launch over n_frames * (tile_hi - tile_lo) tiles + one crop launch */
    uint8_t  pad_[3];
    uint64_t in_bytes, out_bytes;             /* coded bytes of a frame; w * h * (6 | 3)                            */
    uint64_t in_stride_min, out_stride_min;   /* those, rounded up to 16                                            */
    uint64_t scratch_bytes;                   /* per-stream scratch the call holds (so a caller can size its batches) */
} t3_frames_window_plan;
int t3hip_frames_window_plan(uint64_t n_raw_words, uint32_t n_frames, const t3_cfg* cfg, uint32_t fw, uint32_t fh,
                             uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, int out_fmt, t3_frames_window_plan* out);   /* host only */
int t3hip_decode_frames_window_async(const void* d_in9, uint64_t n_in, uint64_t in_stride, uint32_t n_frames, const t3_cfg* cfg,
                                     uint64_t n_raw_words, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                     void* d_out, uint64_t out_stride, int out_fmt, uint32_t* d_verdict /* 2 * n_frames */, void* stream);
int t3hip_decode_frames_window(const void* in9, uint64_t n_in, uint64_t in_stride, uint32_t n_frames, const t3_cfg* cfg,
                               uint64_t n_raw_words, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                               void* out, uint64_t out_stride, int out_fmt, int* frame_rc /* n_frames */);
int t3hip_decode_images_async(const void* d_in9, uint64_t n_in, uint64_t in_stride, uint32_t n_frames, const t3_cfg* cfg,
                              int sub, int centered, uint8_t* d_rgb, uint64_t out_stride, uint32_t* d_verdict, void* stream);

/* ---- image front end: the reference's top-level flow (old/include/io_image.hpp:237-337) on device buffers ----
 * Parity unpinned like the rest of io_image.hpp (restated from the text).  An RGB8 image of any size is brought to the standard
 * resolution of its subword mode (std_res_for: 7680x4320, 3840x2160, 1920x1080, 1280x720, 854x480 for 27/24/21/18/15) by
 * resize_rgb_nn (:102-124) and, when `centered` and sub != 27, centred on the 7680x4320 canvas (blit_center_rgb :125-140).
 *   geometry : host only.  target = std_res_for(sub); centered && sub != 27: frame = 7680x4320, target at centered_window(sub);
 *              else frame = target at (0, 0).  Invalid sub: T3_E_ARG.
 *   resize   : dst pixel (x, y) = src pixel (floor((2x + 1) * sw / (2 * dw)), floor((2y + 1) * sh / (2 * dh))) -- the reference's
 *              (int)((x + 0.5) * (double)sw / dw), equal to it for sides below 2^16; a side >= 2^16 is T3_E_ARG.  sw <= 0 or
 *              sh <= 0: the destination is zeroed, as the reference leaves it.
 *   compose  : resize (only if sw x sh != target) and the centring blit in ONE kernel, the frame (fw * fh * 3 bytes) written once.
 *   encode_image : compose into a per-stream scratch, then what t3hip_encode_rgb_dev does with fw * fh pixels.
 *   decode_image : the target-sized RGB image out of such a frame = t3hip_decode_window_async on the geometry above
 *                  (n_raw_words = fw * fh / 2, the window = the target), RGB out (tw * th * 3 bytes); the resize is not undone.
 * Device pointers: destinations 4-byte aligned, sources any alignment.  _dev entries are asynchronous on `stream`. */
int t3hip_image_geometry(int sub, int centered, int* fw, int* fh, int* x0, int* y0, int* tw, int* th);
int t3hip_resize_rgb_nn_dev(const uint8_t* d_src, int sw, int sh, uint8_t* d_dst, int dw, int dh, void* stream);
int t3hip_resize_rgb_nn(const uint8_t* src, int sw, int sh, uint8_t* dst, int dw, int dh);
int t3hip_image_compose_dev(const uint8_t* d_src, int sw, int sh, int sub, int centered, uint8_t* d_frame_rgb, void* stream);
int t3hip_image_compose(const uint8_t* src, int sw, int sh, int sub, int centered, uint8_t* frame_rgb);
int t3hip_encode_image_dev(const uint8_t* d_src, int sw, int sh, int sub, int centered, const t3_cfg* cfg,
                           void* d_out9, uint64_t cap_words, uint64_t* n_out, void* stream);
int t3hip_decode_image_async(const void* d_in9, uint64_t n_in, const t3_cfg* cfg, int sub, int centered,
                             uint8_t* d_rgb, uint32_t* d_verdict, void* stream);
/* A batch of images of one size through the same flow (a video: one compose launch and one batch encode instead of one of each
 * per frame).  Source f: sw * sh RGB8 pixels at d_src + f * src_stride, at any alignment, src_stride >= sw * sh * 3.  ONE launch
 * composes every frame once into a per-stream scratch at stride r16(fw * fh * 3); then what t3hip_encode_frames_dev does with that
 * scratch, fw * fh units, fmt 2.  Coded frame f, at d_out9 + f * out_stride, equals t3hip_encode_image_dev on source f byte for byte.
 * d_out9 / out_stride: the batch rule (t3hip_frames_plan(0, fw * fh, n_frames, cfg, 2) has the minimum); n_frames as there.  An invalid
 * sub, a side >= 2^16, a null base with bytes to move: T3_E_ARG, before the call asks for a device.  sw <= 0 or sh <= 0 composes zero
 * frames, as the single entry does.  *n_out_words: coded words of ONE frame.  t3hip_encode_images: host buffers, the same strides. */
int t3hip_encode_images_dev(const uint8_t* d_src, int sw, int sh, uint64_t src_stride, uint32_t n_frames, int sub, int centered,
                            const t3_cfg* cfg, void* d_out9, uint64_t out_stride, uint64_t* n_out_words, void* stream);
int t3hip_encode_images(const uint8_t* src, int sw, int sh, uint64_t src_stride, uint32_t n_frames, int sub, int centered,
                        const t3_cfg* cfg, void* out9, uint64_t out_stride, uint64_t* n_out_words);

/* ---- repair of a FIXED coded frame in place: corrected codewords on the wire, no pixels ------------------------------------
 * An archive of T3P6 / T3V6 payloads or a relay that forwards frames wants the damaged STREAM back clean, before errors accumulate past
 * t in some block -- without decoding to pixels, encoding again and writing a second coded buffer, and without one uncorrectable
 * block spoiling its tile.  The repaired frame R' of a received FIXED frame R (a received byte is always taken mod 27):
 *   body block within t = (26 - k_b) / 2 symbols of a codeword (the decoders' rule: L = deg sigma = #roots <= t): that codeword,
 *                    scrambled, as canonical bytes 0..26 -- all 26 positions, data and parity alike
 *   any other body block: byte for byte as received, bytes above 26 included
 *   beacon slots     the symbol the encoder writes there;   tail (behind the body, up to the frame's last word): 0
 *   header           never touched by the device entry; the synchronous entries rewrite it to t3hip_header_encode(cfg, n_raw_words) when
 *                    it decodes (RS + CRC-12) and differs
 *   everything else  R' = R; nothing outside the frame's 9 * n_in bytes is written, and bytes behind the frame's own words (n_in larger
 *                    than the plan's) stay.  A clean canonical frame is a fixed point (no store); repair(repair(R)) = repair(R).
 * flags: T3_REPAIR_WRITE; without it the call is a dry run -- the same verdict words, no byte stored.
 * t3hip_repair_plan is host only and launches nothing.  path 1: repair_fixed_kernel (one k on all bands, no beacon; 1-D and 2-D alike,
 * the interleave acts on data symbols ahead of the band split; 2-D rows of a multiple of 4 symbols, the decoders' own split); path 0:
 * repair_generic_kernel (everything else: per-band k, beacon, other 2-D rows; one lane per block).
 * COMPAT (its parity is not a code its decoder corrects) and RAW mode (no parity): T3_E_ARG; the FIXED limits of the decoders apply.
 * t3hip_repair_frame_async: no synchronisation, in place; d_io9 at any EVEN address.  Bad arguments are refused before a device is
 * asked for.  Device words, zeroed and written by the call on `stream`:
 *   d_verdict[0] = header differs (the rule of t3hip_decode_frame_async)     d_verdict[1] = uncorrectable blocks
 *   d_verdict[2] = blocks changed         d_verdict[3] = bytes whose value differs between R and R' (canonicalised, beacon and tail bytes
 *                                                         count; the header does not)
 * t3hip_repair_profile_dev parses the header on the host as t3hip_decode_profile_dev does (seen->mode must be T3_MODE_FIXED on entry),
 * repairs the body, then the header, and synchronises.  T3_OK, T3_E_RS (some block uncorrectable; the rest is repaired), T3_E_HEADER
 * (nothing written) or T3_E_ARG; counts[1..3] as above, counts[0] = 1 if header bytes were rewritten (a dry run: would be).  The header
 * is rewritten from its own three RS codewords and 12 zero symbols -- the bytes t3hip_header_encode gives for the configuration the
 * frame was encoded with.  Beacon slots get t3hip_beacon_symbol(profile, superframe_words % 5, 0), what the encoder writes; no header
 * carries superframe_words, so these entries take it from `seen` as the caller passes it (t3hip_cfg_default: the encoder's default).
 * t3hip_repair_profile: the same on a host buffer -- one upload, and one download only when T3_REPAIR_WRITE is set and something changed. */
#define T3_REPAIR_WRITE 1u
typedef struct t3_repair_plan {
    uint8_t  path;               /* 1: the fused kernel; 0: the generic kernel                                   */
    uint8_t  pad_[3];
    uint32_t n_tiles;            /* tiles (path 1) / workgroups' worth of blocks (path 0) of the launch           */
    uint32_t blocks_per_tile;    /* 9 * 52 (path 1); 256 (path 0)                                                 */
    uint32_t pad2_;
    uint64_t in_bytes;           /* 9 * coded words of the frame                                                  */
} t3_repair_plan;
int t3hip_repair_plan(uint64_t n_raw_words, const t3_cfg* cfg, t3_repair_plan* out);
int t3hip_repair_frame_async(void* d_io9, uint64_t n_in, const t3_cfg* cfg, uint64_t n_raw_words, uint32_t flags,
                             uint32_t* d_verdict /* 4 words */, void* stream);
int t3hip_repair_profile_dev(void* d_io9, uint64_t n_in, t3_cfg* seen, uint32_t flags, uint32_t counts[4], void* stream);
int t3hip_repair_profile(void* io9, uint64_t n_in, t3_cfg* seen, uint32_t flags, uint32_t counts[4]);

/* ---- repair of a batch of equal FIXED frames in place ---------------------------------------------------------------------------------
 * n_frames frames of one cfg and one n_raw_words; frame f starts f * stride bytes behind frame 0.  What a call does to frame f -- its
 * bytes and its four words -- is what the single-frame entry above does to that frame alone; a damaged frame changes neither the words
 * nor the bytes of its neighbours.  d_io9 EVEN, stride EVEN and >= 9 * n_in (no multiple of 16 asked for: the frames of a T3V6 payload
 * read into one buffer, 9 * words apart, are a batch whenever that is even); n_in: the coded words of ONE frame, at least the plan's --
 * words behind the frame's own stay, and the bytes of a stride behind 9 * n_in are never read or written.
 * n_frames = 0: T3_OK, nothing launched, nothing written; 1: the single-frame entry (the stride is not looked at); more than 65535:
 * T3_E_ARG.  t3hip_repair_frames_plan is host only and launches nothing:
 *   one_launch = 1   exactly where t3hip_repair_plan says path 1 and n_frames >= 2: ONE memset of the 16 * n_frames verdict bytes, ONE
 *                    header compare over all frames, ONE launch of repair_frames_kernel over the tile space n_frames * tiles_per_frame
 *                    (that product < 2^31, else T3_E_ARG).  Such a batch runs that way or is refused, never silently as a loop.
 *   one_launch = 0   path 0 (per-band k, beacon, 2-D rows that are no multiple of 4): a loop of the single-frame body inside the call.
 * t3hip_repair_frames_async: no synchronisation; d_verdict[4 f .. 4 f + 3] = the four words of t3hip_repair_frame_async for frame f.
 * Refusals in the order of the single-frame entries: bad arguments (T3_E_ARG), then n_in below the plan's word count (T3_E_HEADER),
 * then T3_E_NODEVICE.
 * t3hip_repair_frames_dev extends t3hip_repair_profile_dev to the batch (seen->mode must be T3_MODE_FIXED on entry): ONE strided copy
 * fetches the 90 header bytes of every frame, each header is parsed on the host.  A frame whose header does not decode (or names a
 * framing the frame's n_in words cannot hold): frame_rc[f] = T3_E_HEADER, counts[4 f ..] = 0, not touched.  The other frames are cut
 * into maximal runs of consecutive frames whose headers decode to one configuration, one n_raw_words and one scrambler table -- normally
 * ONE run --, each run one batched body repair; then every frame's header is rewritten from its own three RS codewords and 12 zeros
 * where it differs (T3_REPAIR_WRITE), ONE download brings the 16 * n_frames verdict bytes, ONE synchronisation.  frame_rc[f]: T3_OK,
 * T3_E_RS or T3_E_HEADER; counts[4 f ..]: those of t3hip_repair_profile_dev for the frame; *seen: from the first frame whose header
 * decoded.  Returns T3_OK when the call went through whatever the frames returned, T3_E_HEADER only if no frame's header decodes.
 * t3hip_repair_frames: the same on a host buffer (any address; stride >= 9 * n_in) -- one upload of the frames' bytes, and one download
 * only when T3_REPAIR_WRITE is set and something changed. */
typedef struct t3_repair_frames_plan {
    uint32_t n_frames, tiles_per_frame;   /* tiles_per_frame = t3_repair_plan.n_tiles of one frame                       */
    uint8_t  one_launch;                  /* 1: ONE repair launch over n_frames * tiles_per_frame tiles                  */
    uint8_t  path;                        /* t3_repair_plan.path of one frame                                            */
    uint8_t  pad_[6];
    uint64_t in_bytes, stride_min;        /* 9 * coded words of one frame; that rounded up to even                       */
} t3_repair_frames_plan;
int t3hip_repair_frames_plan(uint64_t n_raw_words, uint32_t n_frames, const t3_cfg* cfg, t3_repair_frames_plan* out);
int t3hip_repair_frames_async(void* d_io9, uint64_t n_in, uint64_t stride, uint32_t n_frames, const t3_cfg* cfg, uint64_t n_raw_words,
                              uint32_t flags, uint32_t* d_verdict /* 4 * n_frames words */, void* stream);
int t3hip_repair_frames_dev(void* d_io9, uint64_t n_in, uint64_t stride, uint32_t n_frames, t3_cfg* seen, uint32_t flags,
                            uint32_t* counts /* 4 * n_frames */, int* frame_rc /* n_frames */, void* stream);
int t3hip_repair_frames(void* io9, uint64_t n_in, uint64_t stride, uint32_t n_frames, t3_cfg* seen, uint32_t flags,
                        uint32_t* counts /* 4 * n_frames */, int* frame_rc /* n_frames */);

/* ---- repair with erasures: received bytes above 26 are known-bad positions -----------------------------------------------------------
 * A coded byte is a symbol only up to 26.  Every decoder and the plain repair above take a received byte mod 27; that matches the
 * reference and throws information away: a byte of 27..255 is known to be damaged, and where.  RS(26,k), r = 26 - k parity symbols,
 * corrects e unknown errors and s known-bad positions while 2 e + s <= r.  These entries use that; a receiver that knows a symbol is
 * lost (a demodulator flag, a hole in a file) says so by writing any byte above 26 there, 0xFF for instance.
 * The rule, for a body block of a FIXED frame as the repair's index map places its 26 positions on the wire (band-serial, beacon slots
 * skipped):
 *   E = the positions whose received byte is above 26, s = |E|.
 *   The block is ACCEPTED iff a codeword c of RS(26, k_b) exists with 2 e + s <= r, e = the number of positions outside E where c
 *   differs from the descrambled received symbol.  Such a c is unique (two of them would differ in at most 2 e + s <= r < r + 1
 *   positions).  Accepted: all 26 wire bytes become c, scrambled, as canonical bytes 0..26.
 *   Otherwise the block stays byte for byte as received, bytes above 26 included, and counts as uncorrectable.
 *   s = 0 is the plain repair's rule: on a frame without a body-block byte above 26 these entries write the same bytes and the same
 *   words [0..3] as t3hip_repair_frame_async.
 *   s > 0 is the pure criterion, and it is NOT a superset of the plain repair's: where the residue mod 27 of a flagged byte happens to
 *   be right, the plain repair may accept a block this rule refuses -- RS(26,24) with one flagged byte and one error elsewhere has
 *   2 * 1 + 1 > 2.  That is the price of not trusting a byte known to be bad.
 * Beacon-slot bytes, the tail, the header (its bytes above 26 are still reduced mod 27 by the host parser; header erasures are not
 * handled), dry runs (T3_REPAIR_WRITE absent), alignment (any EVEN address), the order of refusals (arguments, then a truncated stream,
 * then the device) and the COMPAT and RAW-mode refusals: exactly as the plain repair's section states them.  t3hip_repair_plan serves
 * unchanged -- same paths, same tiles; path 1 runs erasure_fixed_kernel, path 0 erasure_generic_kernel.  A repaired buffer holds whole
 * codewords, so this repair followed by any decoder or window decode is erasure decoding for every output format.
 * t3hip_repair_erasures_frame_async: no synchronisation.  Six device words, zeroed and written by the call on `stream`:
 *   [0..3] those of t3hip_repair_frame_async ([1] counts every refused block, flagged or not)
 *   [4] = body blocks holding at least one byte above 26          [5] = how many of those were accepted
 * t3hip_repair_erasures_profile_dev / _profile: the header handling, return codes and one-upload / one-download behaviour of
 * t3hip_repair_profile_dev / _profile; counts[1..5] as above.
 * Block level, FIXED arithmetic only, no scrambler: bytes above 26 among the 26 symbols are erasures.  Accepted: the codeword in place,
 * its first k symbols to data_k, ok = 1.  Refused: the block AND data_k untouched, ok = 0 -- stricter than the errors-only block entries,
 * which leave a refused block partially modified.  _host: one block, no device; returns 1 / 0 / T3_E_ARG. */
int t3hip_repair_erasures_frame_async(void* d_io9, uint64_t n_in, const t3_cfg* cfg, uint64_t n_raw_words, uint32_t flags,
                                      uint32_t* d_verdict /* 6 words */, void* stream);
int t3hip_repair_erasures_profile_dev(void* d_io9, uint64_t n_in, t3_cfg* seen, uint32_t flags, uint32_t counts[6], void* stream);
int t3hip_repair_erasures_profile(void* io9, uint64_t n_in, t3_cfg* seen, uint32_t flags, uint32_t counts[6]);
int t3hip_rs_decode_blocks_erasures_dev(int k, uint8_t* d_code26, uint64_t n_blocks, uint8_t* d_data_k, uint8_t* d_ok, void* stream);
int t3hip_rs_decode_blocks_erasures(int k, uint8_t* code26_inout, uint64_t n_blocks, uint8_t* data_k, uint8_t* ok);
int t3hip_rs_decode_block_erasures_host(int k, uint8_t* code26_inout, uint8_t* data_k);

/* ---- repair with erasures of a batch of equal FIXED frames in place ---------------------------------------------------------------------
 * The batch section above with the rule of "repair with erasures", six words per frame.
 * Per frame: what a call does to frame f -- its bytes and its six words d_verdict[6 f .. 6 f + 5] -- is what
 * t3hip_repair_erasures_frame_async does to that frame alone (the _dev and host forms: what t3hip_repair_erasures_profile_dev does).  A
 * damaged frame changes neither the words nor the bytes of its neighbours; the bytes of a stride behind 9 * n_in are neither read nor
 * written; words behind 6 * n_frames are not written.
 * Plan: t3hip_repair_frames_plan serves unchanged, as t3hip_repair_plan serves the single-frame erasure entries -- the same one_launch,
 * path, tiles_per_frame and stride_min.
 * Addresses, n_frames and refusals are exactly those of the plain batch section: base EVEN, stride EVEN and >= 9 * n_in (no multiple of
 * 16 asked for); n_frames = 0: T3_OK, nothing launched, nothing written, null pointers allowed; 1: the single-frame erasure entry (the
 * stride is not looked at); more than 65535: T3_E_ARG.  Order: bad arguments (T3_E_ARG), then n_in below the plan's word count
 * (T3_E_HEADER), then T3_E_NODEVICE.  COMPAT and RAW mode: T3_E_ARG.
 *   one_launch = 1   (path 1 and n_frames >= 2; n_frames * tiles_per_frame < 2^31, else T3_E_ARG): ONE memset of the 24 * n_frames
 *                    verdict bytes, ONE header compare over all frames (era_hdr_frames_kernel, word 6 f), ONE launch of
 *                    erasure_frames_kernel over the tile space n_frames * tiles_per_frame.  Such a batch runs that way or is refused,
 *                    never silently as a loop.
 *   one_launch = 0   path 0 (per-band k, beacon, 2-D rows that are no multiple of 4): a loop of the single-frame erasure body inside the
 *                    call; frame f's six words go to d_verdict + 6 f.
 * t3hip_repair_erasures_frames_dev extends t3hip_repair_frames_dev (seen->mode must be T3_MODE_FIXED on entry): ONE strided copy fetches
 * the 90 header bytes of every frame, each header is parsed on the host; the frames are cut into maximal runs of consecutive frames of
 * one configuration, one n_raw_words and one scrambler table, each run one batched body repair; headers are rewritten from their own
 * three codewords and 12 zeros where they differ and T3_REPAIR_WRITE is set; ONE download of the 24 * n_frames verdict bytes, ONE
 * synchronisation.  counts[6 f] = 1 if frame f's header was rewritten (a dry run: would be), counts[6 f + 1 .. 6 f + 5] the kernel's
 * words; frame_rc[f]: T3_OK, T3_E_RS or T3_E_HEADER -- a T3_E_HEADER frame is untouched and its six counts are 0.  Return value and
 * *seen as in the plain batch entry.
 * t3hip_repair_erasures_frames: the same on a host buffer -- one upload of the frames' bytes at an even device stride, and one download
 * only when T3_REPAIR_WRITE is set and something changed. */
int t3hip_repair_erasures_frames_async(void* d_io9, uint64_t n_in, uint64_t stride, uint32_t n_frames, const t3_cfg* cfg,
                                       uint64_t n_raw_words, uint32_t flags, uint32_t* d_verdict /* 6 * n_frames words */, void* stream);
int t3hip_repair_erasures_frames_dev(void* d_io9, uint64_t n_in, uint64_t stride, uint32_t n_frames, t3_cfg* seen, uint32_t flags,
                                     uint32_t* counts /* 6 * n_frames */, int* frame_rc /* n_frames */, void* stream);
int t3hip_repair_erasures_frames(void* io9, uint64_t n_in, uint64_t stride, uint32_t n_frames, t3_cfg* seen, uint32_t flags,
                                 uint32_t* counts /* 6 * n_frames */, int* frame_rc /* n_frames */);

/* ---- decode with erasures: FIXED frames with received bytes above 26 taken as known-bad positions, the input read-only ---------------
 * "Repair with erasures" followed by a decoder is erasure decoding in two calls, and it needs a coded buffer the caller may write.  These
 * entries decode straight from a buffer that is `const` and NEVER written -- a mapped T3V6 payload, a frame another stream still reads.
 * The rule is the block rule of "repair with erasures", word for word, for a body block as the decoders' index map places it (band-serial,
 * beacon slots skipped):
 *   E = the positions whose received byte is above 26, s = |E|.
 *   The block is ACCEPTED iff a codeword c of RS(26, k_b) exists with 2 e + s <= r, e = the number of positions outside E where c
 *   differs from the descrambled received symbol.
 *   Accepted: the output carries the first k_b symbols of c, descrambled, wherever the plain decoder would carry the block's data symbols.
 *   Refused: the block counts in word [1]; output units that depend on it are unspecified, as they are for an uncorrectable block in
 *   t3hip_decode_frame_async -- in the one-k 1-D framing its pixel tile and nothing else.  A refused block is NOT retried under the
 *   mod-27 rule: RS(26,24) with one flagged byte and one error elsewhere is refused here although a decoder run on the bytes mod 27 may
 *   accept it (the price stated in "repair with erasures").
 *   Beacon-slot bytes and tail bytes are stepped over whatever they hold.  The header compare is the streaming decoder's: a header byte
 *   above 26 sets word [0]; header erasures are not handled.
 * Four device words, zeroed and written by the call on `stream`:
 *   [0] header differs (the rule of t3hip_decode_frame_async)      [1] refused blocks, flagged or not
 *   [2] body blocks holding at least one byte above 26             [3] how many of those were accepted
 * On a frame without a body-block byte above 26 the output bytes and words [0], [1] are those of t3hip_decode_frame_async /
 * t3hip_decode_rgb_async, and [2] = [3] = 0.
 * fmt: 0 raw Word27 (9 bytes), 1 PixelYCbCrQuant (6 bytes), 2 RGB8 (3 bytes); fmt 1 and 2 produce 2 * n_raw_words pixels.
 * t3hip_decode_erasures_plan is host only and launches nothing:
 *   path 1   exactly where the fused pixel decoder serves a frame: one k on all bands, 1-D, beacon optional (slot < 9, period >= 2),
 *            fmt 1 or 2, n_raw_words > 0.  ONE memset of the 16 verdict bytes and ONE launch of decode_era_px_kernel.  Such a frame runs
 *            that way or is refused (T3_E_ARG: d_out not 16-byte aligned), never silently as path 0.
 *   path 0   everything else the FIXED decoders accept (raw words, per-band k, 2-D, odd 2-D rows), all on `stream`: a device copy of the
 *            frame's 9 * n_in bytes into a per-stream scratch of the context, the erasure repair body on that copy, the streaming decoder
 *            on the copy.  Words [1], [2], [3] are the repair's words 1, 4, 5 -- the rule's, not the count of the decoder that runs on
 *            the repaired copy --, word [0] the header compare's.
 *   COMPAT and RAW mode: T3_E_ARG, as the repairs refuse them.
 * t3hip_decode_erasures_frame_async: no synchronisation.  d_in9 at any EVEN address; d_out as t3hip_decode_frame_async asks (pixels:
 * even) and 16-byte aligned on path 1; cap_units below the plan's out_units: T3_E_CAPACITY.  Refusals in the repair entries' order: bad
 * arguments and T3_E_CAPACITY, then n_in below the plan's word count (T3_E_HEADER), then T3_E_NODEVICE -- all before a device is asked for.
 * t3hip_decode_erasures_profile_dev parses the header on the host as t3hip_decode_profile_dev does (seen->mode must be T3_MODE_FIXED on
 * entry), decodes, and synchronises once to read the words.  T3_OK, T3_E_RS (word [1] != 0; the output is written all the same),
 * T3_E_HEADER (nothing written), T3_E_CAPACITY or T3_E_ARG; counts = the four words, [0] always 0 there.
 * t3hip_decode_erasures_profile: the same on host buffers -- one upload of the frame, one download of the output.
 * Measured (profiles/decode_erasures/notes.md; one 8K RS(26,20) frame, pixels, against repair-with-erasures followed by
 * t3hip_decode_frame_async): 124 against 215 us clean, 161 against 350 us with 0..3 trit errors per block; 13 % SLOWER (2.5 ms) on a frame
 * whose blocks mostly hold bytes above 26.  Not measured: path 0, RGB8, beacon frames. */
typedef struct t3_decode_erasures_plan {
    uint8_t  path;            /* 1: one launch of the fused erasure decoder; 0: private copy + erasure repair + the plain decoder */
    uint8_t  pad_[3];
    uint32_t n_tiles;         /* path 1: tiles of the launch; path 0: 0 */
    uint64_t in_bytes;        /* 9 * coded words of the frame */
    uint64_t out_units;       /* words (fmt 0) or 2 * n_raw_words pixels (fmt 1, 2) */
    uint64_t scratch_bytes;   /* path 0: the private copy (in_bytes rounded up to 16); path 1: 0 */
} t3_decode_erasures_plan;
int t3hip_decode_erasures_plan(uint64_t n_raw_words, const t3_cfg* cfg, int fmt, t3_decode_erasures_plan* out);
int t3hip_decode_erasures_frame_async(const void* d_in9, uint64_t n_in, const t3_cfg* cfg, uint64_t n_raw_words, void* d_out,
                                      uint64_t cap_units, uint64_t* n_out, int fmt, uint32_t* d_verdict /* 4 words */, void* stream);
int t3hip_decode_erasures_profile_dev(const void* d_in9, uint64_t n_in, t3_cfg* seen, void* d_out, uint64_t cap_units,
                                      uint64_t* n_out, int fmt, uint32_t counts[4], void* stream);
int t3hip_decode_erasures_profile(const void* in9, uint64_t n_in, t3_cfg* seen, void* out, uint64_t cap_units,
                                  uint64_t* n_out, int fmt, uint32_t counts[4]);

/* ---- decode with erasures of a batch of equal FIXED frames, the input read-only ---------------------------------------------------------
 * "Decode with erasures" over N frames of one size and one configuration (video: a mapped T3V6 payload) in one call: frame f is read
 * f * in_stride bytes behind frame 0 and written f * out_stride bytes behind d_out; four words per frame.
 * Per frame: frame f's words d_verdict[4 f .. 4 f + 3] are those of t3hip_decode_erasures_frame_async on that frame alone; its output at
 * d_out + f * out_stride equals that entry's output outside the pixel tiles of refused blocks (inside them it is unspecified, as there).
 * A damaged frame changes neither its neighbours' words nor their output.  The input is NEVER written: no byte of a frame, no byte of a
 * stride gap.  Bytes of an output stride behind out_bytes are not written; verdict words behind 4 * n_frames are not written.
 * Addresses: input base EVEN, in_stride EVEN and at least 9 * n_in (the repair batches' rule; no multiple of 16 asked for).  Output base
 * 16-byte aligned, out_stride a multiple of 16 and at least out_stride_min, on both paths.  A null base for bytes that would be moved, or
 * a null d_verdict with n_frames > 0: T3_E_ARG.
 * n_frames: 0 -- T3_OK, nothing launched, nothing written, null pointers allowed; 1 -- the single-frame entry (strides are not looked at,
 * the output rule is that entry's); more than 65535, or n_frames * frame.n_tiles >= 2^31 on the one-launch path: T3_E_ARG.
 * Order of refusals: bad arguments (T3_E_ARG), then n_in below the plan's word count (T3_E_HEADER), then T3_E_NODEVICE -- all before a
 * device is asked for.  COMPAT and RAW mode: T3_E_ARG.
 *   one_launch = 1   (frame.path == 1 and n_frames >= 2; one k on all bands, 1-D, beacon optional, fmt 1 or 2): ONE memset of the
 *                    16 * n_frames verdict bytes and ONE launch of decode_era_frames_px<R, RGB, BCN> over the tile space
 *                    n_frames * frame.n_tiles (t3_decode_era_frames.hip; the header compare of every frame is part of that launch).  Such
 *                    a batch runs that way or is refused, never silently as the loop.
 *   one_launch = 0   (raw words out, per-band k, 2-D): a loop of the single-frame body inside the call, all on `stream`, whose order makes
 *                    reusing the per-stream scratch (scratch_bytes: one frame's private copy) safe.  Frame f's words go to
 *                    d_verdict + 4 f; what the single-frame entry refuses, the batch refuses with the same code.
 * t3hip_decode_erasures_frames_plan is host only and launches nothing.  t3hip_decode_erasures_frames_async does not synchronise.
 * t3hip_decode_erasures_frames_dev (model: t3hip_repair_erasures_frames_dev; seen->mode must be T3_MODE_FIXED on entry; n_in < 10 is
 * T3_E_HEADER): ONE strided copy fetches the 90 header bytes of every frame and each header is parsed on the host; the frames are cut into
 * maximal runs of consecutive frames of one configuration, one n_raw_words and one scrambler table, each run one batched body decode
 * without an in-kernel header compare; ONE download of the verdict words, ONE synchronisation.  counts[4 f] is always 0,
 * counts[4 f + 1 .. 4 f + 3] are the kernel's words.  frame_rc[f]: T3_OK, T3_E_RS (word [1] != 0; the output is written all the same),
 * T3_E_HEADER (the header does not decode, names a framing the frame's n_in words do not hold, or another unit count than the batch's:
 * that frame's output span is untouched, its counts 0) or T3_E_CAPACITY (the frame's units exceed cap_units: nothing written for it).
 * Return value, *seen and *n_out follow t3hip_decode_frames: T3_OK when the call itself went through, whatever the frames' own codes;
 * T3_E_HEADER, with nothing written, when no frame's header decodes; *seen and *n_out (units of ONE frame, also what T3_E_CAPACITY asks
 * for) come from the first header that decodes.  cap_units * unit bytes <= out_stride.
 * t3hip_decode_erasures_frames: the same on host buffers (any base, in_stride >= 9 * n_in, out_stride >= cap_units * unit bytes) -- one
 * upload of the frames' bytes at an even device stride, the _dev entry, one download of the output spans (one per run of decoded frames
 * when a frame in between was refused: a refused frame's span in `out` stays untouched).  The caller's input array is not written.
 * Measured (profiles/decode_erasures_frames/notes.md; RS(26,20), pixels, one call against a loop of the single-frame entry, mean us):
 * 16 frames of 854 x 480 -- 41 against 204 clean, 51 against 241 with 0..3 trit errors per block, 560 against 1476 on frames whose blocks
 * mostly hold bytes above 26; 8 frames of 1920 x 1080 -- 74 against 168, 93 against 199, 1304 against 1565.  Not measured: the loop path
 * (one_launch = 0), RGB8, beacon batches, the _dev and host entries. */
typedef struct t3_decode_erasures_frames_plan {
    t3_decode_erasures_plan frame;            /* the plan of ONE frame                                  */
    uint32_t n_frames;
    uint8_t  one_launch, pad_[3];             /* 1: frame.path == 1 and n_frames >= 2                   */
    uint64_t in_stride_min;                   /* frame.in_bytes rounded up to even                      */
    uint64_t out_bytes, out_stride_min;       /* out_units * (9|6|3); that rounded up to 16             */
    uint64_t scratch_bytes;                   /* per-stream scratch the call holds (loop path: one frame's) */
} t3_decode_erasures_frames_plan;
int t3hip_decode_erasures_frames_plan(uint64_t n_raw_words, uint32_t n_frames, const t3_cfg* cfg, int fmt, t3_decode_erasures_frames_plan* out);
int t3hip_decode_erasures_frames_async(const void* d_in9, uint64_t n_in, uint64_t in_stride, uint32_t n_frames, const t3_cfg* cfg,
                                       uint64_t n_raw_words, void* d_out, uint64_t out_stride, int fmt,
                                       uint32_t* d_verdict /* 4 * n_frames */, void* stream);
int t3hip_decode_erasures_frames_dev(const void* d_in9, uint64_t n_in, uint64_t in_stride, uint32_t n_frames, t3_cfg* seen,
                                     void* d_out, uint64_t out_stride, uint64_t cap_units /* per frame */, uint64_t* n_out, int fmt,
                                     uint32_t* counts /* 4 * n_frames */, int* frame_rc /* n_frames */, void* stream);
int t3hip_decode_erasures_frames(const void* in9, uint64_t n_in, uint64_t in_stride, uint32_t n_frames, t3_cfg* seen,
                                 void* out, uint64_t out_stride, uint64_t cap_units, uint64_t* n_out, int fmt,
                                 uint32_t* counts, int* frame_rc);

/* ---- decode a window with erasures: a pixel window of a FIXED frame, bytes above 26 as known-bad positions, the input read-only ----------
 * "Window decode" joined with "decode with erasures".  The window is the window entry's, word for word: the frame's 2 * n_raw_words decoded
 * pixels are read as rows of fw; output pixel (x, y), 0 <= x < w, 0 <= y < h, is stream pixel (y0 + y) * fw + x0 + x; a row at or beyond
 * fh, or a pixel behind the stream, is an all-zero record in either format.  The block rule is that of "decode with erasures", word for
 * word; a refused block is not retried mod 27.  out_fmt 1 = PixelYCbCrQuant (6 bytes), 2 = RGB8 (3 bytes; bit-identical to
 * t3hip_quant_to_rgb_dev on the window's pixels).
 * Four device words, zeroed and then written by the call on `stream`:
 *   [0] header differs      [1] refused blocks      [2] blocks holding a byte above 26      [3] of those, the accepted ones
 * Words [1..3] count AMONG THE BLOCKS THAT WERE DECODED: on a tile range a refused or flagged block in a tile the window does not touch is
 * neither decoded nor counted.  Window pixels that come from the pixel tile of a refused block are unspecified; every other window byte
 * equals the crop of what t3hip_decode_erasures_frame_async gives for the same input.
 * t3hip_decode_erasures_window_plan is host only and launches nothing:
 *   path 1   exactly where t3hip_decode_erasures_plan says path 1 for fmt 1 / 2 (one k on all bands, 1-D, beacon optional, n_raw_words > 0):
 *            ONE launch of decode_era_window_px<R, RGB, BCN> (t3_decode_era_window.hip), which writes every window pixel straight from its
 *            tile -- no scratch, no crop launch.  Without a beacon the launch covers the tiles [win.tile_lo, win.tile_hi) only; with one
 *            (win.tile_range == 0) it covers every tile of the frame.  win.tile_hi == win.tile_lo on a tile range: no window position is in
 *            the stream, nothing is decoded, the call does the header compare only, words [1..3] are 0 and the window is zeroed.  A frame
 *            whose plan says path 1 runs as that one launch or is refused, never silently as path 0.
 *   path 0   everything else the FIXED decoders accept (per-band k, 2-D, odd 2-D rows): a device copy of the frame into a per-stream
 *            scratch, the erasure repair body on the copy, t3hip_decode_window_async's whole-frame body on the repaired copy (the frame
 *            decoded into a second scratch, the window cut from it), the scrambler taken as the repair takes it.  Words [1], [2], [3] are
 *            the repair's words 1, 4, 5 over the WHOLE frame (all of it was decoded), word [0] the repair's header compare.
 *   zero_fill   some window position maps to no stream pixel (y0 + h > fh, or the last existing window row ends behind the stream): the
 *            call then issues one hipMemsetAsync of out_bytes on `stream` ahead of the launch, else none.
 *   COMPAT, RAW mode, fw == 0, x0 + w > fw, out_fmt other than 1 / 2: T3_E_ARG.  w * h == 0: T3_OK, nothing launched, d_verdict untouched.
 * t3hip_decode_erasures_window_async: no synchronisation.  d_in9 at any EVEN address, never written; d_out 4-byte aligned.  Order of
 * refusals: bad arguments (T3_E_ARG), then n_in below the plan's word count (T3_E_HEADER), then T3_E_NODEVICE -- all before a device is
 * asked for.
 * t3hip_decode_erasures_window_dev follows t3hip_decode_erasures_profile_dev: seen->mode must be T3_MODE_FIXED on entry, n_in < 10 is
 * T3_E_HEADER, the header is parsed on the host (*seen updated once it decodes, n_raw_words from it), the body decoded without an in-kernel
 * header compare, one synchronisation to read the words.  T3_OK, T3_E_RS (word [1] != 0; the window is written all the same), T3_E_HEADER
 * (nothing written) or T3_E_ARG; counts[0] is always 0.
 * t3hip_decode_erasures_window: the same on host buffers -- one upload of the frame, one download of w * h * (6 | 3) bytes.  The caller's
 * input is not written.
 * Measured: profiles/decode_erasures_window/notes.md. */
typedef struct t3_decode_erasures_window_plan {
    t3_window_plan win;        /* what t3hip_window_plan says for the same arguments (tile_range, tile_lo/hi, first_px, n_px) */
    uint8_t  path;             /* 1: ONE launch of decode_era_window_px; 0: private copy + erasure repair + window decode of the copy */
    uint8_t  zero_fill;        /* 1: some window position maps to no stream pixel (row >= fh or behind the stream): the output is zeroed first */
    uint8_t  pad_[2];
    uint32_t tiles_launched;   /* path 1: tile_hi - tile_lo on a tile range, else the frame's tiles; path 0: 0 */
    uint64_t in_bytes;         /* 9 * coded words of the frame */
    uint64_t out_bytes;        /* w * h * (6 | 3) */
    uint64_t scratch_bytes;    /* path 0: the private copy + the frame's decoded pixels; a lower bound -- for n_in == the plan's word
                                  count, without the call's 128 bytes of work words; path 1: 0 */
} t3_decode_erasures_window_plan;
int t3hip_decode_erasures_window_plan(uint64_t n_raw_words, const t3_cfg* cfg, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0,
                                      uint32_t w, uint32_t h, int out_fmt, t3_decode_erasures_window_plan* out);
int t3hip_decode_erasures_window_async(const void* d_in9, uint64_t n_in, const t3_cfg* cfg, uint64_t n_raw_words, uint32_t fw, uint32_t fh,
                                       uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, void* d_out, int out_fmt,
                                       uint32_t* d_verdict /* 4 words */, void* stream);
int t3hip_decode_erasures_window_dev(const void* d_in9, uint64_t n_in, t3_cfg* seen, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0,
                                     uint32_t w, uint32_t h, void* d_out, int out_fmt, uint32_t counts[4], void* stream);
int t3hip_decode_erasures_window(const void* in9, uint64_t n_in, t3_cfg* seen, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0,
                                 uint32_t w, uint32_t h, void* out, int out_fmt, uint32_t counts[4]);

/* ---- decode a window with erasures of a batch of equal FIXED frames: the same pixel window out of every frame, the input read-only -------
 * "Decode a window with erasures" over N frames of one size and one configuration (a viewer or cropper on a read-only mapped T3V6 payload
 * whose damaged bytes are flagged above 26) in one call; four words per frame.
 * Per frame: frame f is read f * in_stride bytes behind frame 0 and written f * out_stride bytes behind d_out.  Its words
 * d_verdict[4 f .. 4 f + 3] are exactly those of t3hip_decode_erasures_window_async on that frame alone (they count AMONG THE DECODED
 * BLOCKS only); its window bytes equal that entry's, except inside the pixel tiles of refused blocks (unspecified, as there).  A damaged
 * frame changes neither its neighbours' words nor their bytes.  The input is NEVER written: no byte of a frame, no byte of a stride gap.
 * Output bytes of a stride behind out_bytes are never written, not by the zero-fill either; verdict words behind 4 * n_frames are never
 * written.
 * Addresses: input base EVEN, in_stride EVEN and at least 9 * n_in (the repair batches' rule).  Output, n_frames >= 2: base 16-byte
 * aligned, out_stride a multiple of 16 and at least out_stride_min, on both paths (this keeps every frame's window base 4-byte aligned, as
 * the single-frame entry asks).  A null base for bytes that would be moved, or a null d_verdict with n_frames > 0: T3_E_ARG.
 * n_frames: 0 -- T3_OK, nothing launched, nothing written, null pointers allowed; 1 -- the single-frame entry (strides are not looked at,
 * the output rule is that entry's 4-byte rule); more than 65535, or n_frames * frame.tiles_launched >= 2^31 on the one-launch path:
 * T3_E_ARG.  w * h == 0: T3_OK, nothing launched, d_verdict untouched.  COMPAT, RAW mode, fw == 0, x0 + w > fw, out_fmt other than 1 / 2:
 * T3_E_ARG from the plan.
 * Order of refusals at a call: bad arguments (T3_E_ARG), then n_in below the plan's word count (T3_E_HEADER), then T3_E_NODEVICE -- all
 * before a device is asked for.
 *   one_launch = 1   exactly when frame.path == 1, n_frames >= 2 and frame.tiles_launched > 0: ONE hipMemsetAsync of the 16 * n_frames
 *                    verdict bytes; where frame.zero_fill, ONE hipMemset2DAsync of width out_bytes, pitch out_stride and height n_frames
 *                    (the stride gaps stay untouched); ONE launch of decode_era_frames_window_px<R, RGB, BCN>
 *                    (t3_decode_era_frames_window.hip) over n_frames * frame.tiles_launched tickets, the header compare of every frame
 *                    part of it.  Such a batch runs that way or is refused, never silently as the loop.
 *   one_launch = 0   path 0 (per-band k, 2-D, odd 2-D rows), or a tile range with tile_hi == tile_lo (only the header compare and the
 *                    zero window remain): a loop of the single-frame window body inside the call, frame by frame on `stream`, whose
 *                    order makes reusing the per-stream scratch safe.  Frame f's words go to d_verdict + 4 f; the refusals and their
 *                    codes are the single-frame entry's.
 * t3hip_decode_erasures_frames_window_plan is host only and launches nothing.  t3hip_decode_erasures_frames_window_async does not
 * synchronise.
 * t3hip_decode_erasures_frames_window_dev (model: t3hip_decode_erasures_frames_dev; the argument checks first; seen->mode must be
 * T3_MODE_FIXED on entry; n_in < 10 is T3_E_HEADER; the device is asked for after that): ONE strided copy fetches the 90 header bytes of
 * every frame and each header is parsed on the host (a header whose framing the window plan refuses does not count); the frames are cut
 * into maximal runs of consecutive frames of one configuration, one n_raw_words and one scrambler table -- the window fixes the output
 * size, so frames of different unit counts may share a call -- each run one batched body without an in-kernel header compare; ONE
 * download of the verdict words, ONE synchronisation.  counts[4 f] is always 0, counts[4 f + 1 .. 4 f + 3] are the kernel's words.
 * frame_rc[f]: T3_OK, T3_E_RS (word [1] != 0; the window is written all the same) or T3_E_HEADER (that frame's output span is untouched,
 * its counts 0).  Return value: T3_OK when the call itself went through, whatever the frames' own codes; T3_E_HEADER, with nothing
 * written, when no frame's header decodes.  *seen comes from the first header that counts.  w * h == 0: the headers are still parsed and
 * frame_rc set, nothing is launched.
 * t3hip_decode_erasures_frames_window: the same on host buffers (any base, in_stride >= 9 * n_in, out_stride >= out_bytes) -- one upload
 * of the frames' bytes at an even device stride, the _dev entry at a device stride of out_bytes rounded up to 16, one download per run of
 * decoded frames (a refused frame's span in `out` stays untouched), one synchronisation.  The caller's input array is not written.
 * Measured (profiles/decode_erasures_frames_window/notes.md; RS(26,20), centred windows, one call against a loop of the single-frame
 * entry, mean us, pixels / RGB8): 16 frames of 854 x 480, window 427 x 240 -- 30 / 32 against 191 / 211 clean, 37 / 39 against 235 / 256
 * with 0..3 trit errors per block, 297 / 301 against 1480 / 1499 with mostly flagged blocks; 8 frames of 1920 x 1080, window 854 x 480 --
 * 52 / 49 against 142 / 146, 62 / 63 against 157 / 159, 651 / 659 against 842 / 854; 4 frames of 8K, window 854 x 480 -- 63 / 66 against
 * 96 / 100, 83 / 91 against 120 / 129, 1189 / 1196 against 1286 / 1299.  Against t3hip_decode_frames_window_async (the plain rule, no
 * erasures) the new entry is NOT faster with trit errors on the two larger batches: 62.4 against 60.4 (1080p, pixels), 62.9 against 62.9
 * (1080p, RGB8), 83.0 against 83.4 (8K, pixels), 90.7 against 84.3 (8K, RGB8: 8 % slower); it is 7 to 9 us faster on the small batch and
 * on clean RGB8 and 8K frames.  Not measured: the loop path (one_launch = 0), beacon batches, the _dev and host entries. */
typedef struct t3_decode_erasures_frames_window_plan {
    t3_decode_erasures_window_plan frame;     /* the plan of ONE frame; every frame shares it                  */
    uint32_t n_frames;
    uint8_t  one_launch, pad_[3];             /* 1: frame.path == 1, n_frames >= 2 and frame.tiles_launched > 0 */
    uint32_t tiles_launched;                  /* one_launch: n_frames * frame.tiles_launched, else 0            */
    uint32_t pad2_;
    uint64_t in_stride_min;                   /* frame.in_bytes rounded up to even                              */
    uint64_t out_bytes, out_stride_min;       /* w * h * (6 | 3); that rounded up to 16                         */
    uint64_t scratch_bytes;                   /* one launch: 0; loop: one frame's (frame.scratch_bytes)         */
} t3_decode_erasures_frames_window_plan;
int t3hip_decode_erasures_frames_window_plan(uint64_t n_raw_words, uint32_t n_frames, const t3_cfg* cfg, uint32_t fw, uint32_t fh,
                                             uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, int out_fmt,
                                             t3_decode_erasures_frames_window_plan* out);
int t3hip_decode_erasures_frames_window_async(const void* d_in9, uint64_t n_in, uint64_t in_stride, uint32_t n_frames, const t3_cfg* cfg,
                                              uint64_t n_raw_words, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0, uint32_t w,
                                              uint32_t h, void* d_out, uint64_t out_stride, int out_fmt,
                                              uint32_t* d_verdict /* 4 * n_frames */, void* stream);
int t3hip_decode_erasures_frames_window_dev(const void* d_in9, uint64_t n_in, uint64_t in_stride, uint32_t n_frames, t3_cfg* seen,
                                            uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, void* d_out,
                                            uint64_t out_stride, int out_fmt, uint32_t* counts /* 4 * n_frames */,
                                            int* frame_rc /* n_frames */, void* stream);
int t3hip_decode_erasures_frames_window(const void* in9, uint64_t n_in, uint64_t in_stride, uint32_t n_frames, t3_cfg* seen,
                                        uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, void* out,
                                        uint64_t out_stride, int out_fmt, uint32_t* counts, int* frame_rc);

/* ---- measurement aid: a plain streaming kernel (16 bytes per lane, four loads in flight) that reads n_read and writes n_write
 * bytes: the part's ceiling for a codec launch's byte volumes (profiles/copy_ceiling.py).  16-byte aligned buffers. */
int t3hip_diag_stream_copy_dev(const void* d_src, uint64_t n_read, void* d_dst, uint64_t n_write, int blocks_per_cu /* < 0: non-temporal */, void* stream);

/* ---- timing helper: HIP events on the caller's stream --------------------------------
 * These events only time.  They are created without the system-scope fence of a default HIP event, so recording one orders nothing
 * and makes nothing visible: not to the host, not to another device, not to another stream.  Do not wait on them for data
 * (hipStreamWaitEvent, or reading a buffer after t3hip_event_elapsed_ms alone); read results after a stream or device
 * synchronisation. */
int t3hip_event_create(void** ev);
int t3hip_event_record(void* ev, void* stream);
int t3hip_event_elapsed_ms(void* ev_start, void* ev_stop, float* ms);   /* synchronises on stop */
int t3hip_event_destroy(void* ev);

#ifdef __cplusplus
}
#endif
#endif /* T3HIP_H */
