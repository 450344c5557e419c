// ternary_codec_v6.hpp — C++17 drop-in for the Word27 hot path of the reference's
// old/include/ternary_image_codec_v6_min.hpp (OLD), implemented on MI355X through libt3hip.so (include/t3hip.h).
//
// Same names, layouts and call signatures as the reference for everything its callers touch on this path
// (old/src/main.cpp:15-27, old/include/io_image.hpp:240-246, include/io_image.hpp:286-310, t3v/t3p writers):
// the types are ABI-identical (Word27 = 9 bytes, PixelYCbCrQuant = 6 bytes), the functions take and fill the same
// std::vector arguments and return the same bool.  What is different, by design:
//   * the arithmetic runs in HIP kernels; there is no CPU implementation behind these functions.  If libt3hip.so has no
//     usable gfx950 device every function returns false and t3::last_status() tells why (T3_E_NODEVICE).
//   * EncoderConfig / DecoderConfigSeen carry one extra field, `mode` (T3_MODE_COMPAT = byte-exact with the reference,
//     bugs included; T3_MODE_FIXED = the self-consistent v6c variant that actually round-trips).
//   * encode_frame / decode_frame fuse pack+encode and decode+unpack into single launches (north-star conveniences).
// Link with -lt3hip (ternary-image-codec_amd/libt3hip.so).
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <random>
#include <vector>

#include "t3hip.h"

// ---- symbols and words (OLD:21-31, 666-674) -------------------------------------------------------------
using UTrit = uint8_t;   // 0..2
using GF27 = uint8_t;    // 0..26
static constexpr int TRITS_PER_WORD = 27, SYM_PER_WORD = 9, NUM_BANDS = 9;
inline GF27 pack3(UTrit a, UTrit b, UTrit c) { return (GF27)(a + 3 * b + 9 * c); }
inline std::array<UTrit, 3> unpack3(GF27 s) { return {(UTrit)(s % 3), (UTrit)(s / 3 % 3), (UTrit)(s / 9 % 3)}; }

struct Word27 { std::array<GF27, SYM_PER_WORD> sym{}; };
struct PixelYCbCrQuant { uint16_t Yq = 0; int16_t Cbq = 0, Crq = 0; };
static_assert(sizeof(Word27) == 9 && sizeof(PixelYCbCrQuant) == 6, "reference ABI");

// ---- profiles, UEP, tiles, scrambler, beacon (OLD:34-114) -------------------------------------------------
enum class ProfileID : uint8_t { RAW_MODE = 0xFF, P1_RS26_24 = 0, P2_RS26_22 = 1, P3_RS26_20 = 2, P4_RS26_18 = 3, P5_RS26_22_2D = 4 };
struct RSParams { uint8_t n = 26, k = 22; };
inline RSParams rs_params_for(ProfileID p) {
    static const uint8_t ks[5] = {24, 22, 20, 18, 22};
    const unsigned i = (unsigned)p;
    return RSParams{26, i < 5 ? ks[i] : (uint8_t)22};
}
struct UEPLayout { std::array<uint8_t, NUM_BANDS> band_profile{}; };
inline void uep_uniform(UEPLayout& u, uint8_t idx = 1) { u.band_profile.fill(idx % 4); }
inline void uep_luma_priority(UEPLayout& u) { u.band_profile.fill(1); u.band_profile[0] = u.band_profile[3] = u.band_profile[6] = 2; }
struct Tile2D { uint16_t w = 0, h = 0; };
struct ScramblerSeed { uint32_t a = 1, b = 1, s0 = 1; };
// one step of the stream scrambler on one symbol (OLD:81-94): the state is stepped first, in uint32 wrap-around arithmetic
inline GF27 scramble_symbol(GF27 s, const ScramblerSeed& seed, uint32_t& st) { return t3hip_scramble_symbol(s, seed.a, seed.b, &st, 0); }
inline GF27 descramble_symbol(GF27 s, const ScramblerSeed& seed, uint32_t& st) { return t3hip_scramble_symbol(s, seed.a, seed.b, &st, 1); }
struct SparseBeaconCfg { uint32_t words_period = 0; uint8_t band_slot = 0; bool enabled = false; };
struct BeaconPayload { ProfileID profile; uint16_t frame_seq_mod; uint8_t health_flags; };
inline GF27 encode_beacon_symbol(const BeaconPayload& b) { return t3hip_beacon_symbol((uint8_t)b.profile, b.frame_seq_mod, b.health_flags); }   // OLD:107-113
enum class CosetID : uint8_t { C0 = 0, C1 = 1, C2 = 2 };

// ---- subword modes and centring (OLD:117-152) ---------------------------------------------------------------
enum class SubwordMode : uint8_t { S27 = 27, S24 = 24, S21 = 21, S18 = 18, S15 = 15 };
inline int payload_len_for(SubwordMode m) { return (int)m; }
struct StdRes { uint16_t w, h; };
inline StdRes std_res_for(SubwordMode m) {
    switch (m) {
        case SubwordMode::S24: return {3840, 2160};
        case SubwordMode::S21: return {1920, 1080};
        case SubwordMode::S18: return {1280, 720};
        case SubwordMode::S15: return {854, 480};
        default: return {7680, 4320};
    }
}
struct ActiveWindow { uint32_t x0, y0, w, h; };
inline ActiveWindow centered_window(SubwordMode m) {
    const StdRes full = std_res_for(SubwordMode::S27), t = std_res_for(m);
    return {(uint32_t)((full.w - t.w) / 2), (uint32_t)((full.h - t.h) / 2), t.w, t.h};
}
inline bool is_valid_subword(SubwordMode m) { const int v = (int)m; return v == 27 || v == 24 || v == 21 || v == 18 || v == 15; }

// ---- contexts (OLD:862-916) -------------------------------------------------------------------------------------
struct EncoderConfig {
    ProfileID profile = ProfileID::P2_RS26_22;
    UEPLayout uep{};
    Tile2D tile{};
    ScramblerSeed seed{1, 1, 1};
    SparseBeaconCfg beacon{};
    uint32_t superframe_words = 8192;
    SubwordMode subword = SubwordMode::S27;
    bool centered = true;
    CosetID coset = CosetID::C0;
    uint8_t mode = T3_MODE_COMPAT;      // build-side: T3_MODE_COMPAT | T3_MODE_FIXED
};
struct DecoderConfigSeen {
    ProfileID profile = ProfileID::P2_RS26_22;
    UEPLayout uep{};
    Tile2D tile{};
    ScramblerSeed seed{1, 1, 1};
    SparseBeaconCfg beacon{};
    SubwordMode subword = SubwordMode::S27;
    bool centered = true;
    CosetID coset = CosetID::C0;
    uint8_t mode = T3_MODE_COMPAT;
};
// (EncoderContext / DecoderContext: below, after GF27Context and RSCodec, which they own as in OLD:885-916)

// ---- header (OLD:155-380) ----------------------------------------------------------------------------------------
struct SuperframeHeader {
    uint16_t magic = 0x0A2; uint8_t version = 1;
    ProfileID profile = ProfileID::P2_RS26_22; UEPLayout uep{}; Tile2D tile{}; ScramblerSeed seed{};
    uint32_t band_map_hash = 0, frame_seq = 0, reserved = 0, crc3m = 0;
    SparseBeaconCfg beacon{}; SubwordMode subword = SubwordMode::S27; bool centered = true; CosetID coset = CosetID::C0;
};
struct HeaderPack { std::array<GF27, 27> symbols{}; };
struct CRC3 {   // OLD:176-205: ternary CRC-12, g = x^12 + x^7 + x^4 + x^3 + 1, twelve zero trits appended to the message
    static constexpr int L = 12;
    static inline void rem12(const std::vector<UTrit>& msg, std::array<UTrit, L>& out) { t3hip_crc12(msg.data(), msg.size(), out.data()); }
};

namespace t3 {
inline int& status_slot() { static thread_local int s = T3_OK; return s; }
inline int last_status() { return status_slot(); }                     // T3_* code of the last call on this thread
inline bool ok(int rc) { status_slot() = rc; return rc == T3_OK; }
inline bool ensure_device(int dev = 0) { return t3hip_is_ready() || ok(t3hip_init(dev)); }

template <class Cfg> inline t3_cfg to_pod(const Cfg& c, uint32_t superframe_words) {
    t3_cfg p; std::memset(&p, 0, sizeof p);
    p.profile = (uint8_t)c.profile;
    for (int i = 0; i < 9; ++i) p.band_profile[i] = c.uep.band_profile[i];
    p.tile_w = c.tile.w; p.tile_h = c.tile.h;
    p.seed_a = c.seed.a; p.seed_b = c.seed.b; p.seed_s0 = c.seed.s0;
    p.beacon_words_period = c.beacon.words_period; p.beacon_band_slot = c.beacon.band_slot; p.beacon_enabled = c.beacon.enabled;
    p.subword = (uint8_t)c.subword; p.centered = c.centered; p.coset = (uint8_t)c.coset; p.mode = c.mode;
    p.superframe_words = superframe_words;
    return p;
}
inline void from_pod(const t3_cfg& p, DecoderConfigSeen& c) {
    c.profile = (ProfileID)p.profile;
    for (int i = 0; i < 9; ++i) c.uep.band_profile[i] = p.band_profile[i];
    c.tile.w = p.tile_w; c.tile.h = p.tile_h;
    c.seed.a = p.seed_a; c.seed.b = p.seed_b; c.seed.s0 = p.seed_s0;
    c.beacon.words_period = p.beacon_words_period; c.beacon.band_slot = p.beacon_band_slot; c.beacon.enabled = p.beacon_enabled != 0;
    c.subword = (SubwordMode)p.subword; c.centered = p.centered != 0; c.coset = (CosetID)p.coset; c.mode = p.mode;
}
}  // namespace t3

// ---- GF(27) and the RS(26,k) block codec (OLD:383-663) ------------------------------------------------------------------
inline GF27 gf27_add(GF27 a, GF27 b) { return t3hip_gf27_add(a, b); }
inline GF27 gf27_sub(GF27 a, GF27 b) { return t3hip_gf27_sub(a, b); }
inline GF27 gf27_mul_poly(GF27 a, GF27 b) { return t3hip_gf27_mul(a, b); }
struct GF27Tables {
    std::array<GF27, 26 * 3> exp{}; std::array<int16_t, 27> log{}; std::array<GF27, 27 * 27> mul{}; std::array<GF27, 27> inv{};
    GF27 primitive = 0;
};
struct GF27Context {
    GF27Tables tab{};
    int order_of(GF27 g) const { if (g == 0 || g == 1) return -1; GF27 x = 1; for (int i = 1; i <= 26; ++i) { x = gf27_mul_poly(x, g); if (x == 1) return i; } return -1; }
    void init() { t3hip_gf27_tables(tab.exp.data(), tab.log.data(), tab.mul.data(), tab.inv.data()); tab.primitive = tab.exp[1]; }   // OLD:436-466 (primitive = 3)
    GF27 add(GF27 a, GF27 b) const { return gf27_add(a, b); }
    GF27 sub(GF27 a, GF27 b) const { return gf27_sub(a, b); }
    GF27 mul(GF27 a, GF27 b) const { return tab.mul[a * 27 + b]; }
    GF27 inv(GF27 a) const { return tab.inv[a]; }
    GF27 pow_alpha(int e) const { return tab.exp[(e % 26 + 26) % 26]; }
    int log(GF27 a) const { return tab.log[a]; }
};
// One block per call, as in the reference: 26 symbols are control data and are coded on the host (t3hip_rs_encode_block_host /
// t3hip_rs_decode_block_host: the parity matrix and decoder the kernels are built from, no launch) -- a caller that walks blocks
// one at a time, like the reference's self-test OLD:1172-1207, pays integer arithmetic, not 10 us per block.  Bulk work goes
// through t3hip_rs_encode_blocks / t3hip_rs_decode_blocks (device) or, for whole frames, encode_profile_from_raw / decode_profile_to_raw.
// `mode` is build-side: T3_MODE_COMPAT = the reference's arithmetic (its parity map, Forney with add), T3_MODE_FIXED = v6c; a codec
// owned by a context follows that context's cfg.mode (mode_ref).
struct RSCodec {
    GF27Context* gf = nullptr; RSParams params{}; std::vector<GF27> g; uint8_t mode = T3_MODE_COMPAT; const uint8_t* mode_ref = nullptr;
    int arithmetic() const { return mode_ref ? *mode_ref : mode; }
    void init(GF27Context* c, RSParams p) { gf = c; params = p; build_gen(); }
    void build_gen() { g.assign((size_t)(params.n - params.k + 1), 0); if (t3hip_rs_generator(params.k, g.data()) != T3_OK) g.assign(1, 1); }   // OLD:501-516
    bool encode_block(const GF27* data_k, GF27* out_n) const { return t3hip_rs_encode_block_host(params.k, arithmetic(), data_k, out_n) == T3_OK; }   // OLD:517-535
    GF27 poly_eval(const std::vector<GF27>& p, GF27 x) const {   // OLD:536-545 (Horner)
        GF27 acc = 0;
        for (int i = (int)p.size() - 1; i >= 0; --i) acc = gf27_add(gf27_mul_poly(acc, x), p[(size_t)i]);
        return acc;
    }
    // OLD:546-662: inout_n corrected in place, out_k only on success
    bool decode_block(GF27* inout_n, GF27* out_k) const { return t3hip_rs_decode_block_host(params.k, arithmetic(), inout_n, out_k) == 1; }
};

// ---- contexts (OLD:885-916): the field tables and the five codecs as members, so reference code that reaches into them
// (ectx.rs_p3.encode_block(...), dctx.gf.mul(...)) compiles unchanged.  The codecs follow cfg.mode / cfg_last_seen.mode.  Unlike the
// reference's (RSCodec::gf is a raw pointer into the owning context, OLD:492) these can be copied: a copy re-binds its own members.
struct EncoderContext {
    GF27Context gf; RSCodec rs_p1, rs_p2, rs_p3, rs_p4, rs_hdr; EncoderConfig cfg;
    EncoderContext() { bind(); uep_uniform(cfg.uep, 1); }
    EncoderContext(const EncoderContext& o) : cfg(o.cfg) { bind(); }
    EncoderContext& operator=(const EncoderContext& o) { cfg = o.cfg; return *this; }
private:
    void bind() {
        gf.init();
        RSCodec* cs[5] = {&rs_p1, &rs_p2, &rs_p3, &rs_p4, &rs_hdr};
        const RSParams ps[5] = {rs_params_for(ProfileID::P1_RS26_24), rs_params_for(ProfileID::P2_RS26_22), rs_params_for(ProfileID::P3_RS26_20), rs_params_for(ProfileID::P4_RS26_18), RSParams{26, 18}};
        for (int i = 0; i < 5; ++i) { cs[i]->init(&gf, ps[i]); cs[i]->mode_ref = &cfg.mode; }
    }
};
struct DecoderContext {
    GF27Context gf; RSCodec rs_p1, rs_p2, rs_p3, rs_p4, rs_hdr; DecoderConfigSeen cfg_last_seen;
    DecoderContext() { bind(); uep_uniform(cfg_last_seen.uep, 1); }
    DecoderContext(const DecoderContext& o) : cfg_last_seen(o.cfg_last_seen) { bind(); }
    DecoderContext& operator=(const DecoderContext& o) { cfg_last_seen = o.cfg_last_seen; return *this; }
private:
    void bind() {
        gf.init();
        RSCodec* cs[5] = {&rs_p1, &rs_p2, &rs_p3, &rs_p4, &rs_hdr};
        const RSParams ps[5] = {rs_params_for(ProfileID::P1_RS26_24), rs_params_for(ProfileID::P2_RS26_22), rs_params_for(ProfileID::P3_RS26_20), rs_params_for(ProfileID::P4_RS26_18), RSParams{26, 18}};
        for (int i = 0; i < 5; ++i) { cs[i]->init(&gf, ps[i]); cs[i]->mode_ref = &cfg_last_seen.mode; }
    }
};

struct HeaderCodec {
    static HeaderPack pack(const SuperframeHeader& h) {
        EncoderConfig c; c.profile = h.profile; c.uep = h.uep; c.tile = h.tile; c.seed = h.seed; c.beacon = h.beacon;
        c.subword = h.subword; c.centered = h.centered; c.coset = h.coset;
        const t3_cfg p = t3::to_pod(c, 0);
        HeaderPack out; t3hip_header_pack(&p, h.frame_seq, h.band_map_hash, out.symbols.data());
        return out;
    }
    static bool check(const HeaderPack& p) { return t3hip_header_check(p.symbols.data()) == 1; }
    static SuperframeHeader unpack(const HeaderPack& p) {
        t3_cfg c; std::memset(&c, 0, sizeof c); uint32_t fs = 0, bh = 0;
        t3hip_header_unpack(p.symbols.data(), &c, &fs, &bh);
        DecoderConfigSeen d; t3::from_pod(c, d);
        SuperframeHeader h; h.magic = (uint16_t)(p.symbols[0] % 27 + 27 * (p.symbols[1] % 27)); h.version = p.symbols[2] % 27;
        h.profile = d.profile; h.uep = d.uep; h.tile = d.tile; h.seed = d.seed; h.beacon = d.beacon;
        h.subword = d.subword; h.centered = d.centered; h.coset = d.coset; h.frame_seq = fs; h.band_map_hash = bh;
        return h;
    }
};

// ---- RAW packer primitives (OLD:675-722) ---------------------------------------------------------------------------------
inline void i2tr(uint32_t v, int w, std::array<UTrit, 27>& d, int s) { for (int i = 0; i < w; ++i) { d[(size_t)(s + i)] = (UTrit)(v % 3); v /= 3; } }
inline uint32_t tr2i(const std::array<UTrit, 27>& d, int w, int s) { uint32_t val = 0, p = 1; for (int i = 0; i < w; ++i) { val += p * d[(size_t)(s + i)]; p *= 3; } return val; }
// One word = 26 trits = one integer below 3^26 < 2^42: the components are digit runs of it (Y: 5 trits, Cb + 40 and Cr + 40: 4 each,
// pixel b 13 trits further up, trit 26 = 0), the nine symbols are its base-27 digits.  Host integer arithmetic, no device: a
// caller that loops these as OLD:728-733 does pays nanoseconds per word.  No clamping, as in the reference: a component enters
// as (uint32 cast) mod 3^width (OLD:675-682, 697-702).
inline void pack_two_pixels(const PixelYCbCrQuant& a, const PixelYCbCrQuant& b, Word27& w) {          // OLD:693-705
    auto px13 = [](const PixelYCbCrQuant& p) -> uint64_t {
        return (uint64_t)((uint32_t)p.Yq % 243u) + 243ull * ((uint32_t)((int)p.Cbq + 40) % 81u) + 19683ull * ((uint32_t)((int)p.Crq + 40) % 81u);
    };
    uint64_t v = px13(a) + 1594323ull * px13(b);                      // 3^13
    for (int s = 0; s < SYM_PER_WORD; ++s) { w.sym[(size_t)s] = (GF27)(v % 27u); v /= 27u; }
}
inline void unpack_two_pixels(const Word27& w, PixelYCbCrQuant& a, PixelYCbCrQuant& b) {            // OLD:706-722 (unpack3 reduces every digit; trit 26 ignored)
    uint64_t v = 0;
    for (int s = SYM_PER_WORD - 1; s >= 0; --s) v = 27u * v + w.sym[(size_t)s] % 27u;
    auto px13 = [](uint64_t u, PixelYCbCrQuant& p) {
        p.Yq = (uint16_t)(u % 243u); p.Cbq = (int16_t)((int)(u / 243u % 81u) - 40); p.Crq = (int16_t)((int)(u / 19683u % 81u) - 40);
    };
    px13(v % 1594323ull, a); px13(v / 1594323ull % 1594323ull, b);
}
// ---- 2-D boustrophedon on a symbol vector (OLD:750-813) --------------------------------------------------------------------
inline void interleave2D_boustrophedon(std::vector<GF27>& syms, Tile2D tile) { if (!t3hip_is_ready()) t3hip_init(0); t3hip_interleave2d(syms.data(), syms.size(), tile.w, tile.h, 0); }
inline void deinterleave2D_boustrophedon(std::vector<GF27>& syms, Tile2D tile) { if (!t3hip_is_ready()) t3hip_init(0); t3hip_interleave2d(syms.data(), syms.size(), tile.w, tile.h, 1); }

// ---- RAW packer (OLD:723-747; `_subword` variants NEWH:113-125 / NEWC:139-155) ------------------------------------
inline bool encode_raw_pixels_to_words(const std::vector<PixelYCbCrQuant>& px, std::vector<Word27>& out) {
    out.clear();
    if (!t3::ensure_device()) return false;
    out.resize((px.size() + 1) / 2);
    return t3::ok(t3hip_pack_pixels(px.data(), px.size(), out.data()));
}
inline bool decode_raw_words_to_pixels(const std::vector<Word27>& in, std::vector<PixelYCbCrQuant>& out) {
    out.clear();
    if (!t3::ensure_device()) return false;
    out.resize(in.size() * 2);
    return t3::ok(t3hip_unpack_words(in.data(), in.size(), out.data()));
}
inline bool encode_raw_pixels_to_words_subword(const std::vector<PixelYCbCrQuant>& px, SubwordMode sub, std::vector<Word27>& out) {
    if (!is_valid_subword(sub)) { t3::status_slot() = T3_E_ARG; return false; }
    return encode_raw_pixels_to_words(px, out);
}
inline bool decode_raw_words_to_pixels_subword(const std::vector<Word27>& in, SubwordMode sub, std::vector<PixelYCbCrQuant>& out) {
    if (!is_valid_subword(sub)) { t3::status_slot() = T3_E_ARG; return false; }
    return decode_raw_words_to_pixels(in, out);
}

// ---- RGB8 <-> quantised YCbCr bridge (old/include/io_image.hpp:17-21,156-195) --------------------------------------------
struct ImageU8 { int w = 0, h = 0, c = 0; std::vector<uint8_t> data; };
inline void rgb_to_quant_stream(const ImageU8& rgb, std::vector<PixelYCbCrQuant>& out) {
    out.clear();
    const size_t n = (size_t)(rgb.w > 0 ? rgb.w : 0) * (size_t)(rgb.h > 0 ? rgb.h : 0);
    if (!n || rgb.data.size() < 3 * n || !t3::ensure_device()) return;
    out.resize(n);
    if (!t3::ok(t3hip_rgb_to_quant(rgb.data.data(), n, out.data()))) out.clear();
}
inline void quant_stream_to_rgb(const std::vector<PixelYCbCrQuant>& q, int w, int h, ImageU8& out) {
    out.w = w; out.h = h; out.c = 3;
    const size_t n = (size_t)(w > 0 ? w : 0) * (size_t)(h > 0 ? h : 0);
    out.data.assign(n * 3, 0);
    const size_t m = q.size() < n ? q.size() : n;                     // io_image.hpp:181: stops when the stream runs out
    if (!m || !t3::ensure_device()) return;
    t3::ok(t3hip_quant_to_rgb(q.data(), m, out.data.data()));
}

// centring blits, io_image.hpp:125-140 and :215-235 (a source wider than the canvas / a window wider than the frame, where the
// reference runs over the row, leaves the zeroed canvas / an all-zero window)
inline void blit_center_rgb(const ImageU8& src, int canvasW, int canvasH, ImageU8& dst) {
    dst.w = canvasW; dst.h = canvasH; dst.c = 3;
    dst.data.assign((size_t)(canvasW > 0 ? canvasW : 0) * (size_t)(canvasH > 0 ? canvasH : 0) * 3, 0);
    if (dst.data.empty() || src.w <= 0 || src.h <= 0 || !t3::ensure_device()) return;
    t3::ok(t3hip_blit_center_rgb(src.data.data(), src.w, src.h, dst.data.data(), canvasW, canvasH));
}
inline void extract_center_q(const std::vector<PixelYCbCrQuant>& q_full, int fullW, int fullH, int subW, int subH, std::vector<PixelYCbCrQuant>& q_sub) {
    q_sub.assign((size_t)(subW > 0 ? subW : 0) * (size_t)(subH > 0 ? subH : 0), PixelYCbCrQuant{});
    if (q_sub.empty() || fullW <= 0 || fullH <= 0 || q_full.size() < (size_t)fullW * (size_t)fullH || !t3::ensure_device()) return;
    t3::ok(t3hip_extract_center_q(q_full.data(), fullW, fullH, q_sub.data(), subW, subH));
}

// ---- image front end, io_image.hpp:102-124, 141-144, 237-337 (memory forms: the path-taking ones need stb) ----------------
inline void resize_rgb_nn(const ImageU8& src, int dstW, int dstH, ImageU8& dst) {
    dst.w = dstW; dst.h = dstH; dst.c = 3;
    dst.data.assign((size_t)(dstW > 0 ? dstW : 0) * (size_t)(dstH > 0 ? dstH : 0) * 3, 0);
    if (dst.data.empty() || src.w <= 0 || src.h <= 0 || src.data.size() < (size_t)src.w * (size_t)src.h * 3 || !t3::ensure_device()) return;
    t3::ok(t3hip_resize_rgb_nn(src.data.data(), src.w, src.h, dst.data.data(), dstW, dstH));
}
inline int pad_even(int w) { return (w % 2 == 0) ? w : (w + 1); }
// image -> RAW words: resize to std_res_for(sub) when the size differs, centre on the S27 canvas when `centered` and sub != S27 (one
// kernel), bridge, pack.  The reference's even-width padding cannot act (the canvas is 7680 wide) and its second attempt is never
// reached (the first returns false only for an invalid `sub`, which fails the second too): both are left out.
inline bool image_to_words_subword(const ImageU8& src, SubwordMode sub, bool centered, std::vector<Word27>& out_words) {
    out_words.clear();
    int fw = 0, fh = 0;
    if (!is_valid_subword(sub) || t3hip_image_geometry((int)sub, centered ? 1 : 0, &fw, &fh, nullptr, nullptr, nullptr, nullptr) != T3_OK) { t3::status_slot() = T3_E_ARG; return false; }
    if (src.w > 0 && src.h > 0 && src.data.size() < (size_t)src.w * (size_t)src.h * 3) { t3::status_slot() = T3_E_ARG; return false; }
    if (!t3::ensure_device()) return false;
    ImageU8 frame; frame.w = fw; frame.h = fh; frame.c = 3; frame.data.assign((size_t)fw * (size_t)fh * 3, 0);
    if (!t3::ok(t3hip_image_compose(src.data.data(), src.w, src.h, (int)sub, centered ? 1 : 0, frame.data.data()))) return false;
    std::vector<PixelYCbCrQuant> q;
    rgb_to_quant_stream(frame, q);
    return encode_raw_pixels_to_words_subword(q, sub, out_words);
}
// RAW words -> image, the reference's three branches (io_image.hpp:318-336): a stream of exactly w * h pixels; an S27-sized stream with
// sub != S27 -> the centre window of sub's standard resolution; else best effort at (w, h)
inline bool words_to_image_subword(const std::vector<Word27>& words, SubwordMode sub, int w, int h, ImageU8& out) {
    std::vector<PixelYCbCrQuant> q;
    if (!decode_raw_words_to_pixels_subword(words, sub, q)) return false;
    const StdRes big = std_res_for(SubwordMode::S27), tgt = std_res_for(sub);
    const size_t need_sub = (size_t)(w > 0 ? w : 0) * (size_t)(h > 0 ? h : 0);
    if (q.size() != need_sub && q.size() == (size_t)big.w * big.h && sub != SubwordMode::S27) {
        std::vector<PixelYCbCrQuant> q_sub;
        extract_center_q(q, big.w, big.h, tgt.w, tgt.h, q_sub);
        quant_stream_to_rgb(q_sub, w, h, out);
        return true;
    }
    quant_stream_to_rgb(q, w, h, out);
    return true;
}

// ---- subword trit streams (OLD:834-859) and wire packings (include/ternary_packing.hpp, namespace tpack) --------------
inline void extract_subword_stream_from_words(const std::vector<Word27>& words, int N, std::vector<UTrit>& out) {
    out.clear();
    if (N < 1 || N > 27 || !t3::ensure_device()) return;
    out.resize(words.size() * (size_t)N);
    if (!t3::ok(t3hip_subword_extract(words.data(), words.size(), N, out.data()))) out.clear();
}
inline void build_words_from_subword_stream(const std::vector<UTrit>& in, int N, std::vector<Word27>& out, UTrit fill = 0) {
    out.clear();
    if (N < 1 || N > 27 || !t3::ensure_device()) return;
    out.resize((size_t)t3hip_subword_words(in.size(), N));
    uint64_t nw = 0;
    if (!t3::ok(t3hip_subword_build(in.data(), in.size(), N, fill, out.data(), out.size(), &nw))) { out.clear(); return; }
    out.resize((size_t)nw);
}
namespace tpack {
inline void ut_to_base243(const std::vector<UTrit>& in, std::vector<uint8_t>& out) {   // TPACK:28-38
    out.clear();
    if (!t3::ensure_device()) return;
    out.resize((size_t)t3hip_base243_bytes(in.size()));
    uint64_t nb = 0;
    if (!t3::ok(t3hip_base243_pack(in.data(), in.size(), out.data(), out.size(), &nb))) { out.clear(); return; }
    out.resize((size_t)nb);
}
inline bool base243_to_ut(const std::vector<uint8_t>& in, std::vector<UTrit>& out) {     // TPACK:40-50
    out.clear();
    if (in.size() < 4 || !t3::ensure_device()) return false;
    out.resize(5 * (in.size() - 4));
    uint64_t nt = 0;
    if (!t3::ok(t3hip_base243_unpack(in.data(), in.size(), out.data(), out.size(), &nt))) { out.clear(); return false; }
    out.resize((size_t)nt);
    return true;
}
inline void words_to_bytes(const std::vector<Word27>& words, std::vector<uint8_t>& out) {  // TPACK:53-58
    out.clear();
    if (!t3::ensure_device()) return;
    out.resize(words.size() * 9);
    if (!t3::ok(t3hip_mod27_bytes((const uint8_t*)words.data(), out.size(), out.data()))) out.clear();
}
inline void bytes_to_words(const std::vector<uint8_t>& in, std::vector<Word27>& out) {     // TPACK:60-65
    out.clear();
    if (in.size() % 9 != 0 || !t3::ensure_device()) return;
    out.resize(in.size() / 9);
    if (!t3::ok(t3hip_mod27_bytes(in.data(), in.size(), (uint8_t*)out.data()))) out.clear();
}
}  // namespace tpack

// ---- profile encode / decode (OLD:995-1169) --------------------------------------------------------------------------
inline bool encode_profile_from_raw(const std::vector<Word27>& in, std::vector<Word27>& out, EncoderContext& ectx) {
    out.clear();
    if (!t3::ensure_device()) return false;
    const t3_cfg c = t3::to_pod(ectx.cfg, ectx.cfg.superframe_words);
    const uint64_t cap = t3hip_encoded_words(in.size(), &c);
    out.resize(cap); uint64_t n = 0;
    const bool good = t3::ok(t3hip_encode_profile(in.data(), in.size(), &c, out.data(), cap, &n));
    out.resize(good ? n : 0);
    return good;
}
// ---- single-word subword helpers (OLD:816-833): control data, host code --------------------------------------------------
inline void extract_subword_trits_from_word(const Word27& w, int N, std::array<UTrit, 27>& out) {   // all 27 trits; N unused, as in the reference
    for (int s = 0; s < SYM_PER_WORD; ++s) {
        const std::array<UTrit, 3> d = unpack3(w.sym[(size_t)s]);
        out[(size_t)(3 * s)] = d[0]; out[(size_t)(3 * s + 1)] = d[1]; out[(size_t)(3 * s + 2)] = d[2];
    }
    (void)N;
}
// T[i] = inN[i] for i < N, fill after; pack3 without reduction, so out-of-range trits pass through as in the reference.  N is clamped
// to [0, 27]: the reference writes past its 27-trit array for N > 27 (and before it for N < 0).
inline void inject_subword_trits_into_word(const UTrit* inN, int N, Word27& w, UTrit fill = 0) {
    N = N < 0 ? 0 : N > TRITS_PER_WORD ? TRITS_PER_WORD : N;
    std::array<UTrit, 27> T{};
    for (int i = 0; i < N; ++i) T[(size_t)i] = inN[i];
    for (int i = N; i < TRITS_PER_WORD; ++i) T[(size_t)i] = fill;
    for (int s = 0; s < SYM_PER_WORD; ++s) w.sym[(size_t)s] = pack3(T[(size_t)(3 * s)], T[(size_t)(3 * s + 1)], T[(size_t)(3 * s + 2)]);
}

// ---- the reference decoder's stages one at a time (OLD:918-993; decode_profile_to_raw below fuses them) -------------------------------
// Stage 1, header words -> header: six words are control data, decoded on the host with the codec's own arithmetic (RSCodec::decode_block).
// cursor is left alone when fewer than six words remain and advanced by six before decoding otherwise (also on a false); `out` is
// written only on success.  A codec other than RS(26,18) returns false (T3_E_ARG): the reference overruns its 18-symbol buffers for k > 18.
inline bool read_and_decode_header_from_words(const std::vector<Word27>& words, size_t& cursor, SuperframeHeader& out, RSCodec& rs_hdr) {
    if (cursor + 6 > words.size()) return false;
    GF27 A[26], B[26];
    for (int i = 0; i < 52; ++i) (i < 26 ? A[i] : B[i - 26]) = words[cursor + (size_t)(i / 9)].sym[(size_t)(i % 9)];
    cursor += 6;
    if (rs_hdr.params.n != 26 || rs_hdr.params.k != 18) { t3::status_slot() = T3_E_ARG; return false; }
    GF27 a18[18]{}, b18[18]{};
    if (!rs_hdr.decode_block(A, a18)) return false;
    if (!rs_hdr.decode_block(B, b18)) return false;
    HeaderPack hp{};
    for (int i = 0; i < 18; ++i) hp.symbols[(size_t)i] = a18[i];
    for (int i = 0; i < 9; ++i) hp.symbols[(size_t)(18 + i)] = b18[i];
    if (!HeaderCodec::check(hp)) return false;
    out = HeaderCodec::unpack(hp);
    return true;
}
// Stage 2, in place: only hdr.seed is read (descramble_words_kernel through t3hip_descramble_words).
inline void descramble_words_inplace(std::vector<Word27>& words, const SuperframeHeader& hdr) {
    if (words.empty() || !t3::ensure_device()) return;
    t3::ok(t3hip_descramble_words(words.data(), words.size(), hdr.seed.a, hdr.seed.b, hdr.seed.s0));
}
// Stage 3 on a descrambled body: band b = slot b of every word (beacon words of the beacon slot skipped), decoded with r1..r4 by
// hdr.uep.band_profile[b] % 4, each codec with its own k and arithmetic() (stage_decode_kernel through t3hip_demap_rsdecode_bands).
// On the first block that does not decode it returns false with out_syms holding the symbols of the blocks before it, as the
// reference does.  A codec a band uses other than RS(26, 18 | 20 | 22 | 24) returns false (T3_E_ARG).
inline bool demap_and_rsdecode_bands_from_words(const std::vector<Word27>& body, std::vector<GF27>& out_syms, const SuperframeHeader& hdr,
                                                RSCodec& r1, RSCodec& r2, RSCodec& r3, RSCodec& r4) {
    out_syms.clear();
    const RSCodec* cs[4] = {&r1, &r2, &r3, &r4};
    uint8_t ks[4], ms[4];
    for (int q = 0; q < 4; ++q) { ks[q] = cs[q]->params.k; ms[q] = (uint8_t)cs[q]->arithmetic(); }
    t3_cfg h; std::memset(&h, 0, sizeof h);
    for (int b = 0; b < NUM_BANDS; ++b) {
        h.band_profile[b] = hdr.uep.band_profile[(size_t)b];
        if (cs[h.band_profile[b] % 4]->params.n != 26) { t3::status_slot() = T3_E_ARG; return false; }
    }
    h.beacon_words_period = hdr.beacon.words_period; h.beacon_band_slot = hdr.beacon.band_slot; h.beacon_enabled = hdr.beacon.enabled ? 1 : 0;
    if (!t3::ensure_device()) return false;
    out_syms.resize((size_t)t3hip_demap_rsdecode_bands_syms(body.size(), &h, ks));
    uint64_t n = 0;
    const int rc = t3hip_demap_rsdecode_bands(body.data(), body.size(), &h, ks, ms, out_syms.data(), out_syms.size(), &n);
    out_syms.resize(rc == T3_OK || rc == T3_E_RS ? (size_t)n : 0);
    return t3::ok(rc);
}

inline bool decode_profile_to_raw(const std::vector<Word27>& in, std::vector<Word27>& out, DecoderContext& dctx) {
    out.clear();
    if (!t3::ensure_device()) return false;
    t3_cfg c = t3::to_pod(dctx.cfg_last_seen, 0);
    out.resize(in.size() + 16); uint64_t n = 0;
    const int rc = t3hip_decode_profile(in.data(), in.size(), &c, out.data(), out.size(), &n);
    t3::from_pod(c, dctx.cfg_last_seen);                 // the header, once decoded, is remembered even if a block fails (OLD:1006-1017)
    out.resize(rc == T3_OK ? n : 0);
    return t3::ok(rc);
}
// pixels -> coded words and back in one launch each (= OLD:723 + OLD:1043, OLD:995 + OLD:735)
inline bool encode_frame(const std::vector<PixelYCbCrQuant>& px, std::vector<Word27>& out, EncoderContext& ectx) {
    out.clear();
    if (!t3::ensure_device()) return false;
    const t3_cfg c = t3::to_pod(ectx.cfg, ectx.cfg.superframe_words);
    const uint64_t cap = t3hip_encoded_words((px.size() + 1) / 2, &c);
    out.resize(cap); uint64_t n = 0;
    const bool good = t3::ok(t3hip_encode_frame(px.data(), px.size(), &c, out.data(), cap, &n));
    out.resize(good ? n : 0);
    return good;
}
inline bool decode_frame(const std::vector<Word27>& in, std::vector<PixelYCbCrQuant>& px, DecoderContext& dctx) {
    px.clear();
    if (!t3::ensure_device()) return false;
    t3_cfg c = t3::to_pod(dctx.cfg_last_seen, 0);
    px.resize(2 * (in.size() + 16)); uint64_t n = 0;
    const int rc = t3hip_decode_frame(in.data(), in.size(), &c, px.data(), px.size(), &n);
    t3::from_pod(c, dctx.cfg_last_seen);
    px.resize(rc == T3_OK ? n : 0);
    return t3::ok(rc);
}

// ---- repair of a FIXED coded frame in place (t3hip.h "repair"): an archive or a relay gets the damaged STREAM back clean -- every block
// within t of a codeword rewritten to that codeword on the wire, parity included, the header to its own codewords -- without decoding to
// pixels and encoding again.  dctx.cfg_last_seen.mode must be T3_MODE_FIXED; the header, once it decodes, is remembered as by
// decode_profile_to_raw.  true: every block is clean now.  false with last_status() == T3_E_RS: some block is beyond repair and stays as
// it was received, the rest is repaired (rep->uncorrectable counts them); T3_E_HEADER: nothing was changed.
// superframe_words: the encoder's EncoderConfig::superframe_words -- the beacon symbol depends on it (OLD:1130) and no header carries it;
// frames without a beacon do not care.
struct RepairReport { uint32_t header_rewritten = 0, uncorrectable = 0, blocks_changed = 0, bytes_changed = 0; };
inline bool repair_profile(std::vector<Word27>& words, DecoderContext& dctx, RepairReport* rep = nullptr, uint32_t superframe_words = EncoderConfig{}.superframe_words) {
    if (rep) *rep = RepairReport{};
    if (!t3::ensure_device()) return false;
    t3_cfg c = t3::to_pod(dctx.cfg_last_seen, superframe_words);
    uint32_t n[4] = {0, 0, 0, 0};
    const int rc = t3hip_repair_profile(words.data(), words.size(), &c, T3_REPAIR_WRITE, n);
    if (rc == T3_OK || rc == T3_E_RS) t3::from_pod(c, dctx.cfg_last_seen);
    if (rep) { rep->header_rewritten = n[0]; rep->uncorrectable = n[1]; rep->blocks_changed = n[2]; rep->bytes_changed = n[3]; }
    return t3::ok(rc);
}

// The same for a batch: `words` holds n_frames coded frames of words.size() / n_frames words each, back to back (a T3V6 payload's frames
// read into one vector), repaired in place by t3hip_repair_frames -- one upload, one batched body repair per run of equal headers (one
// launch where the fused kernel serves the framing), one download when something changed.  (*reps)[f]: frame f's report.  true: every
// frame is clean now.  false with last_status() == T3_E_RS: some frame holds a block beyond repair, T3_E_HEADER: some frame's header
// does not decode and that frame is unchanged -- the other frames are repaired either way, and (*reps)[f] / (*frame_status)[f] (T3_OK,
// T3_E_RS or T3_E_HEADER) tell which.  T3_E_ARG, nothing done: words.size() is no multiple of n_frames, or a frame's byte size (9 x its
// words) is odd -- frames packed back to back then start at odd addresses, which the device entries do not take.
inline bool repair_frames(std::vector<Word27>& words, size_t n_frames, DecoderContext& dctx, std::vector<RepairReport>* reps = nullptr,
                          uint32_t superframe_words = EncoderConfig{}.superframe_words, std::vector<int>* frame_status = nullptr) {
    if (reps) reps->assign(n_frames, RepairReport{});
    if (frame_status) frame_status->assign(n_frames, T3_OK);
    if (n_frames == 0) { t3::status_slot() = words.empty() ? T3_OK : T3_E_ARG; return words.empty(); }
    const size_t per = words.size() / n_frames;
    if (words.size() % n_frames != 0 || n_frames > 65535 || (n_frames > 1 && (per & 1u) != 0)) { t3::status_slot() = T3_E_ARG; return false; }
    if (!t3::ensure_device()) return false;
    t3_cfg c = t3::to_pod(dctx.cfg_last_seen, superframe_words);
    std::vector<uint32_t> n(4 * n_frames, 0u); std::vector<int> rcs(n_frames, T3_OK);
    const int rc = t3hip_repair_frames(words.data(), per, sizeof(Word27) * per, (uint32_t)n_frames, &c, T3_REPAIR_WRITE, n.data(), rcs.data());
    if (rc != T3_OK) return t3::ok(rc);
    t3::from_pod(c, dctx.cfg_last_seen);
    int worst = T3_OK;
    for (size_t f = 0; f < n_frames; ++f) {
        if (reps) { RepairReport& r = (*reps)[f]; r.header_rewritten = n[4 * f]; r.uncorrectable = n[4 * f + 1]; r.blocks_changed = n[4 * f + 2]; r.bytes_changed = n[4 * f + 3]; }
        if (frame_status) (*frame_status)[f] = rcs[f];
        if (rcs[f] == T3_E_HEADER || (rcs[f] != T3_OK && worst == T3_OK)) worst = rcs[f];
    }
    return t3::ok(worst);
}

// ---- repair with erasures (t3hip.h "repair with erasures"): the receiver marks a symbol it knows to be lost with any byte above 26, and a
// block is accepted while 2 e + s <= r (e unknown errors, s marked positions).  The shape, the return rules and the T3_E_ARG cases of
// repair_profile / repair_frames; the report carries the two further counts.
struct ErasureReport { uint32_t header_rewritten = 0, uncorrectable = 0, blocks_changed = 0, bytes_changed = 0, flagged_blocks = 0, flagged_accepted = 0; };
namespace t3 {
inline void to_report(const uint32_t* n, ErasureReport& r) {
    r.header_rewritten = n[0]; r.uncorrectable = n[1]; r.blocks_changed = n[2]; r.bytes_changed = n[3]; r.flagged_blocks = n[4]; r.flagged_accepted = n[5];
}
}  // namespace t3
inline bool repair_erasures_profile(std::vector<Word27>& words, DecoderContext& dctx, ErasureReport* rep = nullptr, uint32_t superframe_words = EncoderConfig{}.superframe_words) {
    if (rep) *rep = ErasureReport{};
    if (!t3::ensure_device()) return false;
    t3_cfg c = t3::to_pod(dctx.cfg_last_seen, superframe_words);
    uint32_t n[6] = {0, 0, 0, 0, 0, 0};
    const int rc = t3hip_repair_erasures_profile(words.data(), words.size(), &c, T3_REPAIR_WRITE, n);
    if (rc == T3_OK || rc == T3_E_RS) t3::from_pod(c, dctx.cfg_last_seen);
    if (rep) t3::to_report(n, *rep);
    return t3::ok(rc);
}

// The batch: n_frames coded frames back to back in `words`, through t3hip_repair_erasures_frames -- one upload, one batched body repair per
// run of equal headers (one launch where the fused kernel serves the framing), one download when something changed.
inline bool repair_erasures_frames(std::vector<Word27>& words, size_t n_frames, DecoderContext& dctx, std::vector<ErasureReport>* reps = nullptr,
                                   uint32_t superframe_words = EncoderConfig{}.superframe_words, std::vector<int>* frame_status = nullptr) {
    if (reps) reps->assign(n_frames, ErasureReport{});
    if (frame_status) frame_status->assign(n_frames, T3_OK);
    if (n_frames == 0) { t3::status_slot() = words.empty() ? T3_OK : T3_E_ARG; return words.empty(); }
    const size_t per = words.size() / n_frames;
    if (words.size() % n_frames != 0 || n_frames > 65535 || (n_frames > 1 && (per & 1u) != 0)) { t3::status_slot() = T3_E_ARG; return false; }
    if (!t3::ensure_device()) return false;
    t3_cfg c = t3::to_pod(dctx.cfg_last_seen, superframe_words);
    std::vector<uint32_t> n(6 * n_frames, 0u); std::vector<int> rcs(n_frames, T3_OK);
    const int rc = t3hip_repair_erasures_frames(words.data(), per, sizeof(Word27) * per, (uint32_t)n_frames, &c, T3_REPAIR_WRITE, n.data(), rcs.data());
    if (rc != T3_OK) return t3::ok(rc);
    t3::from_pod(c, dctx.cfg_last_seen);
    int worst = T3_OK;
    for (size_t f = 0; f < n_frames; ++f) {
        if (reps) t3::to_report(n.data() + 6 * f, (*reps)[f]);
        if (frame_status) (*frame_status)[f] = rcs[f];
        if (rcs[f] == T3_E_HEADER || (rcs[f] != T3_OK && worst == T3_OK)) worst = rcs[f];
    }
    return t3::ok(worst);
}

// ---- decode a window with erasures (t3hip.h "decode a window with erasures"): the w x h window at (x0, y0) of a received frame read as
// rows of fw pixels, bytes above 26 taken as erasures, the caller's words never written.  The shape and return rules of
// repair_erasures_profile; of the report only uncorrectable, flagged_blocks and flagged_accepted are filled, counted among the blocks
// that were decoded.  false with T3_E_RS: some decoded block was refused, `px` holds the window all the same; T3_E_HEADER: `px` is empty.
inline bool decode_window_erasures(const std::vector<Word27>& words, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                   std::vector<PixelYCbCrQuant>& px, DecoderContext& dctx, ErasureReport* rep = nullptr,
                                   uint32_t superframe_words = EncoderConfig{}.superframe_words) {
    if (rep) *rep = ErasureReport{};
    px.clear();
    if (!t3::ensure_device()) return false;
    t3_cfg c = t3::to_pod(dctx.cfg_last_seen, superframe_words);
    std::vector<PixelYCbCrQuant> win((size_t)w * h);
    uint32_t n[4] = {0, 0, 0, 0};
    const int rc = t3hip_decode_erasures_window(words.data(), words.size(), &c, fw, fh, x0, y0, w, h, win.data(), 1, n);
    if (rc == T3_OK || rc == T3_E_RS) { t3::from_pod(c, dctx.cfg_last_seen); px.swap(win); }
    if (rep) { rep->uncorrectable = n[1]; rep->flagged_blocks = n[2]; rep->flagged_accepted = n[3]; }
    return t3::ok(rc);
}

// The batch (t3hip.h "decode a window with erasures of a batch of equal FIXED frames"): n_frames coded frames back to back in `words`, the
// same window out of each, through t3hip_decode_erasures_frames_window -- one upload, one batched launch per run of equal headers where
// the fused kernel serves the framing, one download per run of decoded frames.  px: n_frames windows of w * h records back to back; the
// window of a frame whose header does not decode stays zero and (*frame_status)[f] is T3_E_HEADER.  The shape and return rules of
// repair_erasures_frames; the reports are filled as decode_window_erasures fills its one.
inline bool decode_frames_window_erasures(const std::vector<Word27>& words, size_t n_frames, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                          std::vector<PixelYCbCrQuant>& px, DecoderContext& dctx, std::vector<ErasureReport>* reps = nullptr,
                                          uint32_t superframe_words = EncoderConfig{}.superframe_words, std::vector<int>* frame_status = nullptr) {
    if (reps) reps->assign(n_frames, ErasureReport{});
    if (frame_status) frame_status->assign(n_frames, T3_OK);
    px.clear();
    if (n_frames == 0) { t3::status_slot() = words.empty() ? T3_OK : T3_E_ARG; return words.empty(); }
    const size_t per = words.size() / n_frames;
    if (words.size() % n_frames != 0 || n_frames > 65535) { t3::status_slot() = T3_E_ARG; return false; }
    if (!t3::ensure_device()) return false;
    t3_cfg c = t3::to_pod(dctx.cfg_last_seen, superframe_words);
    const size_t wpx = (size_t)w * h;
    std::vector<PixelYCbCrQuant> win(wpx * n_frames);
    std::vector<uint32_t> n(4 * n_frames, 0u); std::vector<int> rcs(n_frames, T3_OK);
    const int rc = t3hip_decode_erasures_frames_window(words.data(), per, sizeof(Word27) * per, (uint32_t)n_frames, &c, fw, fh, x0, y0, w, h, win.data(),
                                                       sizeof(PixelYCbCrQuant) * wpx, 1, n.data(), rcs.data());
    if (rc != T3_OK) return t3::ok(rc);
    t3::from_pod(c, dctx.cfg_last_seen);
    px.swap(win);
    int worst = T3_OK;
    for (size_t f = 0; f < n_frames; ++f) {
        if (reps) { ErasureReport& r = (*reps)[f]; r.uncorrectable = n[4 * f + 1]; r.flagged_blocks = n[4 * f + 2]; r.flagged_accepted = n[4 * f + 3]; }
        if (frame_status) (*frame_status)[f] = rcs[f];
        if (rcs[f] == T3_E_HEADER || (rcs[f] != T3_OK && worst == T3_OK)) worst = rcs[f];
    }
    return t3::ok(worst);
}

// ---- batches of equal frames (the video loop, old/src/main_video_t3v.cpp:24-26, in one call; t3hip.h "batches of equal frames") ----------
// frames[f] -> coded[f]: the frames are packed into one strided staging vector (16-byte strides) and go through t3hip_encode_frames /
// t3hip_decode_frames -- one upload, one codec launch where the fused single-k kernels serve the framing, one download.  Frames of
// unequal size: false (T3_E_ARG), nothing is encoded.
inline bool encode_frames(const std::vector<std::vector<PixelYCbCrQuant>>& frames, std::vector<std::vector<Word27>>& coded, EncoderContext& ectx) {
    coded.clear();
    if (frames.empty()) return true;
    for (const auto& f : frames) if (f.size() != frames[0].size()) { t3::status_slot() = T3_E_ARG; return false; }
    if (!t3::ensure_device()) return false;
    const t3_cfg c = t3::to_pod(ectx.cfg, ectx.cfg.superframe_words);
    const uint64_t n_px = frames[0].size(); const uint32_t n = (uint32_t)frames.size();
    t3_frames_plan fp;
    if (!t3::ok(t3hip_frames_plan(0, n_px, n, &c, 1, &fp))) return false;
    std::vector<uint8_t> in((size_t)(fp.in_stride_min * n)), out((size_t)(fp.out_stride_min * n));
    for (uint32_t f = 0; f < n; ++f) if (n_px) std::memcpy(in.data() + (size_t)(f * fp.in_stride_min), frames[f].data(), (size_t)fp.in_bytes);
    uint64_t words = 0;
    if (!t3::ok(t3hip_encode_frames(in.data(), n_px, 1, fp.in_stride_min, n, &c, out.data(), fp.out_stride_min, &words))) return false;
    coded.resize(n);
    for (uint32_t f = 0; f < n; ++f) { coded[f].resize((size_t)words); if (words) std::memcpy(coded[f].data(), out.data() + (size_t)(f * fp.out_stride_min), (size_t)(9 * words)); }
    return true;
}
// coded[f] -> frames[f]; frame 0's header sets the configuration (remembered in dctx as decode_frame does).  frame_ok, when given, gets
// one verdict per frame; a frame that does not decode (header or RS block) is left empty.  Returns true when every frame decoded.
inline bool decode_frames(const std::vector<std::vector<Word27>>& coded, std::vector<std::vector<PixelYCbCrQuant>>& frames, DecoderContext& dctx,
                          std::vector<bool>* frame_ok = nullptr) {
    frames.clear(); if (frame_ok) frame_ok->clear();
    if (coded.empty()) return true;
    for (const auto& f : coded) if (f.size() != coded[0].size()) { t3::status_slot() = T3_E_ARG; return false; }
    if (!t3::ensure_device()) return false;
    t3_cfg c = t3::to_pod(dctx.cfg_last_seen, 0);
    const uint64_t n_in = coded[0].size(), cap = 2 * (n_in + 16); const uint32_t n = (uint32_t)coded.size();
    const uint64_t in_stride = (9 * n_in + 15) & ~15ull, out_stride = (6 * cap + 15) & ~15ull;
    std::vector<uint8_t> in((size_t)(in_stride * n)), out((size_t)(out_stride * n));
    for (uint32_t f = 0; f < n; ++f) if (n_in) std::memcpy(in.data() + (size_t)(f * in_stride), coded[f].data(), (size_t)(9 * n_in));
    std::vector<int> rcs(n, T3_E_HEADER); uint64_t n_px = 0;
    const int rc = t3hip_decode_frames(in.data(), n_in, in_stride, n, out.data(), out_stride, cap, 1, &c, &n_px, rcs.data());
    if (rc == T3_OK) t3::from_pod(c, dctx.cfg_last_seen);
    if (!t3::ok(rc)) return false;
    frames.resize(n);
    bool all = true;
    for (uint32_t f = 0; f < n; ++f) {
        const bool good = rcs[f] == T3_OK;
        if (frame_ok) frame_ok->push_back(good);
        if (good) { frames[f].resize((size_t)n_px); if (n_px) std::memcpy(frames[f].data(), out.data() + (size_t)(f * out_stride), (size_t)(6 * n_px)); }
        else { all = false; t3::status_slot() = rcs[f]; }
    }
    return all;
}

// ---- the same window out of every frame of a batch; batches through the image front end (t3hip.h, same section) -----------------------
// These decode with a KNOWN configuration, dctx.cfg_last_seen (a decoder context that remembers a configuration decodes the following
// frames with it), and frames of fw * fh pixels: nothing is read back before the launch.  A frame's header is still compared, and a frame
// whose header does not decode to that configuration and size is reported (frame_ok) and left empty.
namespace t3 {
// coded[f] (equal sizes) -> the w x h window of every frame, out_fmt 1 pixels / 2 RGB8, `unit` bytes per pixel, packed into wins[f]
inline bool frames_window_bytes(const std::vector<std::vector<Word27>>& coded, const t3_cfg& c, uint64_t n_raw, uint32_t fw, uint32_t fh, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h,
                                int out_fmt, std::vector<std::vector<uint8_t>>& wins, std::vector<bool>* frame_ok) {
    wins.clear(); if (frame_ok) frame_ok->clear();
    if (coded.empty()) return true;
    for (const auto& f : coded) if (f.size() != coded[0].size()) { status_slot() = T3_E_ARG; return false; }
    if (!ensure_device()) return false;
    const uint64_t n_in = coded[0].size(); const uint32_t n = (uint32_t)coded.size();
    t3_frames_window_plan fp;
    if (!ok(t3hip_frames_window_plan(n_raw, n, &c, fw, fh, x0, y0, w, h, out_fmt, &fp))) return false;
    const uint64_t in_stride = (9 * n_in + 15) & ~15ull, out_stride = fp.out_stride_min;
    std::vector<uint8_t> in((size_t)(in_stride * n)), out((size_t)(out_stride * n));
    for (uint32_t f = 0; f < n; ++f) if (n_in) std::memcpy(in.data() + (size_t)(f * in_stride), coded[f].data(), (size_t)(9 * n_in));
    std::vector<int> rcs(n, T3_E_HEADER);
    if (!ok(t3hip_decode_frames_window(in.data(), n_in, in_stride, n, &c, n_raw, fw, fh, x0, y0, w, h, out.data(), out_stride, out_fmt, rcs.data()))) return false;
    wins.resize(n);
    bool all = true;
    for (uint32_t f = 0; f < n; ++f) {
        const bool good = rcs[f] == T3_OK;
        if (frame_ok) frame_ok->push_back(good);
        if (good) wins[f].assign(out.begin() + (ptrdiff_t)(f * out_stride), out.begin() + (ptrdiff_t)(f * out_stride + fp.out_bytes));
        else { all = false; status_slot() = rcs[f]; }
    }
    return all;
}
}  // namespace t3
// coded[f], frames of fw x fh pixels -> frames[f] = the w x h window at (x0, y0) (t3hip_decode_frames_window: one upload, one decoder
// launch and one crop launch where the framing has a tile range, one download).  Returns true when every frame decoded.
inline bool decode_frames_window(const std::vector<std::vector<Word27>>& coded, int fw, int fh, int x0, int y0, int w, int h,
                                 std::vector<std::vector<PixelYCbCrQuant>>& frames, DecoderContext& dctx, std::vector<bool>* frame_ok = nullptr) {
    frames.clear(); if (frame_ok) frame_ok->clear();
    if (fw <= 0 || fh < 0 || x0 < 0 || y0 < 0 || w < 0 || h < 0) { t3::status_slot() = T3_E_ARG; return false; }
    const t3_cfg c = t3::to_pod(dctx.cfg_last_seen, 0);
    std::vector<std::vector<uint8_t>> wins;
    const bool all = t3::frames_window_bytes(coded, c, ((uint64_t)fw * (uint64_t)fh + 1) / 2, (uint32_t)fw, (uint32_t)fh, (uint32_t)x0, (uint32_t)y0, (uint32_t)w, (uint32_t)h, 1, wins, frame_ok);
    frames.resize(wins.size());
    for (size_t f = 0; f < wins.size(); ++f) { frames[f].resize(wins[f].size() / sizeof(PixelYCbCrQuant)); if (!wins[f].empty()) std::memcpy(frames[f].data(), wins[f].data(), wins[f].size()); }
    return all;
}
// The image front end over a batch (image_to_words_subword / words_to_image_subword are single frames of RAW words; these are coded frames):
// coded[f], each a frame of sub's geometry (t3hip_image_geometry) -> images[f], the target-sized RGB image (the resize is not undone)
inline bool frames_to_images(const std::vector<std::vector<Word27>>& coded, SubwordMode sub, bool centered, std::vector<ImageU8>& images, DecoderContext& dctx,
                             std::vector<bool>* frame_ok = nullptr) {
    images.clear(); if (frame_ok) frame_ok->clear();
    int fw = 0, fh = 0, x0 = 0, y0 = 0, tw = 0, th = 0;
    if (!is_valid_subword(sub) || t3hip_image_geometry((int)sub, centered ? 1 : 0, &fw, &fh, &x0, &y0, &tw, &th) != T3_OK) { t3::status_slot() = T3_E_ARG; return false; }
    const t3_cfg c = t3::to_pod(dctx.cfg_last_seen, 0);
    std::vector<std::vector<uint8_t>> wins;
    const bool all = t3::frames_window_bytes(coded, c, (uint64_t)fw * (uint64_t)fh / 2, (uint32_t)fw, (uint32_t)fh, (uint32_t)x0, (uint32_t)y0, (uint32_t)tw, (uint32_t)th, 2, wins, frame_ok);
    images.resize(wins.size());
    for (size_t f = 0; f < wins.size(); ++f) if (!wins[f].empty()) { images[f].w = tw; images[f].h = th; images[f].c = 3; images[f].data.swap(wins[f]); }
    return all;
}
// images[f] (one size, RGB8) -> coded[f]: one compose launch (resize to sub's standard resolution where the size differs, centring blit)
// and the batch encoder (t3hip_encode_images).  Images of unequal size: false (T3_E_ARG), nothing is encoded.
inline bool images_to_frames(const std::vector<ImageU8>& images, SubwordMode sub, bool centered, std::vector<std::vector<Word27>>& coded, EncoderContext& ectx) {
    coded.clear();
    if (images.empty()) return true;
    if (!is_valid_subword(sub)) { t3::status_slot() = T3_E_ARG; return false; }
    const int sw = images[0].w, sh = images[0].h;
    const size_t src_bytes = sw > 0 && sh > 0 ? (size_t)sw * (size_t)sh * 3 : 0;
    for (const auto& im : images) if (im.w != sw || im.h != sh || im.data.size() < src_bytes) { t3::status_slot() = T3_E_ARG; return false; }
    if (!t3::ensure_device()) return false;
    const t3_cfg c = t3::to_pod(ectx.cfg, ectx.cfg.superframe_words);
    int fw = 0, fh = 0;
    if (!t3::ok(t3hip_image_geometry((int)sub, centered ? 1 : 0, &fw, &fh, nullptr, nullptr, nullptr, nullptr))) return false;
    const uint32_t n = (uint32_t)images.size();
    t3_frames_plan fp;
    if (!t3::ok(t3hip_frames_plan(0, (uint64_t)fw * (uint64_t)fh, n, &c, 2, &fp))) return false;
    std::vector<uint8_t> in(src_bytes * n), out((size_t)(fp.out_stride_min * n));
    for (uint32_t f = 0; f < n; ++f) if (src_bytes) std::memcpy(in.data() + src_bytes * f, images[f].data.data(), src_bytes);
    uint64_t words = 0;
    if (!t3::ok(t3hip_encode_images(in.data(), sw, sh, src_bytes, n, (int)sub, centered ? 1 : 0, &c, out.data(), fp.out_stride_min, &words))) return false;
    coded.resize(n);
    for (uint32_t f = 0; f < n; ++f) { coded[f].resize((size_t)words); if (words) std::memcpy(coded[f].data(), out.data() + (size_t)(f * fp.out_stride_min), (size_t)(9 * words)); }
    return true;
}

// ---- self-tests with the reference's inputs (OLD:1172-1230) ------------------------------------------------------------
// The reference's own versions return false / false (its encode_block is not an RS encoder and its framings disagree).
// Default: the same inputs through FIXED arithmetic, where both pass.  Compile with -DT3_SELFTEST_REFERENCE_ARITHMETIC to run them
// exactly as the reference does (COMPAT arithmetic, the reference's statements in the reference's order): both then return the
// reference's verdicts, false / false (tests/golden/ref_vectors.json "selftests").
#ifdef T3_SELFTEST_REFERENCE_ARITHMETIC
static constexpr uint8_t T3_SELFTEST_MODE = T3_MODE_COMPAT;
#else
static constexpr uint8_t T3_SELFTEST_MODE = T3_MODE_FIXED;
#endif
inline bool selftest_rs_unit() {   // OLD:1172-1207: same data pattern, error positions and values (std::mt19937 rng(1)); host arithmetic only
    GF27Context gf; gf.init();
    std::mt19937 rng(1);
    for (ProfileID pid : {ProfileID::P1_RS26_24, ProfileID::P2_RS26_22, ProfileID::P3_RS26_20, ProfileID::P4_RS26_18}) {
        RSCodec rs; rs.mode = T3_SELFTEST_MODE; rs.init(&gf, rs_params_for(pid));
        const int n = rs.params.n, k = rs.params.k, t = (n - k) / 2;
        std::vector<GF27> data((size_t)k);
        for (int i = 0; i < k; ++i) data[(size_t)i] = (GF27)((i * 5 + 7) % 27);
        std::vector<GF27> code((size_t)n);
        rs.encode_block(data.data(), code.data());
        std::uniform_int_distribution<int> pos(0, n - 1), val(1, 26);
        std::vector<int> used;
        for (int e = 0; e < t; ++e) {
            int p;
            do { p = pos(rng); } while (std::find(used.begin(), used.end(), p) != used.end());
            used.push_back(p);
            code[(size_t)p] = gf.add(code[(size_t)p], (GF27)val(rng));
        }
        std::vector<GF27> outk((size_t)k);
        if (!rs.decode_block(code.data(), outk.data())) return false;
        if (outk != data) return false;
    }
    return true;
}
inline bool selftest_api_roundtrip() {   // OLD:1208-1230
    std::vector<PixelYCbCrQuant> px(64);
    for (size_t i = 0; i < px.size(); ++i) { px[i].Yq = (uint16_t)(i * 7 % 243); px[i].Cbq = (int16_t)((int)(i * 3 % 81) - 40); px[i].Crq = (int16_t)((int)(i * 5 % 81) - 40); }
    std::vector<Word27> raw, coded, back;
    if (!encode_raw_pixels_to_words(px, raw)) return false;
    EncoderContext e; e.cfg.profile = ProfileID::P2_RS26_22; e.cfg.mode = T3_SELFTEST_MODE; uep_luma_priority(e.cfg.uep);
    if (!encode_profile_from_raw(raw, coded, e)) return false;
    DecoderContext d; d.cfg_last_seen.mode = T3_SELFTEST_MODE;
    if (!decode_profile_to_raw(coded, back, d)) return false;
    const size_t L = std::min(raw.size(), back.size());               // the reference compares the common prefix (OLD:1226-1228)
    return std::memcmp(back.data(), raw.data(), L * 9) == 0;
}
