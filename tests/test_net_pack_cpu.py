"""The operand images of csrc/net_pack.h, unpacked on the CPU.  A stand-alone program packs networks whose weights come from an
integer hash of the element index and writes every image to a file; here each image is taken apart by the layout its comment
documents and must give the weights back (float32 exactly; bf16 as three planes whose float32 sum, smallest first, is the
weight bit for bit), padding must be zero, and the SHA-256 of every image must equal tests/golden/net_pack_digests.json, which
was recorded from the packing loops as they stood inside engine.hip before they moved.  No GPU and no libblackbird_hip.so."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from tests.host_cases import host_compiler
from tests.split_cases import _bf16_nearest, _bits, _widen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "blackbird_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "net_pack_digests.json")

# name: H, W, C, A as the game has them; F, R; the dense width 10 and A = 7 are no multiples of 4 (the head's padding)
SHAPES = {
    "connect4_f16_r0": (6, 7, 3, 7, 16, 0, 10),
    "connect4_f16_r1": (6, 7, 3, 7, 16, 1, 10),
    "connect4_f16_r4": (6, 7, 3, 7, 16, 4, 10),
    "dragonchess_f16_r1": (8, 8, 17, 4032, 16, 1, 10),
    "connect4_f32_r2": (6, 7, 3, 7, 32, 2, 10),
    "connect4_f48_r1": (6, 7, 3, 7, 48, 1, 10),
}
TENSORS = ["conv0_k", "conv0_b", "conv0_bn", "blk_k", "blk_b", "blk_bn", "v_conv_k", "v_conv_b", "v_bn", "v_d1_k", "v_d1_b",
           "v_d2_k", "v_d2_b", "p_conv_k", "p_conv_b", "p_bn", "p_d_k", "p_d_b"]

# ---- the part every packing program shares: hashed weights, files out ----------------------------------------------------------
COMMON = r"""
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
// a float from a fixed integer hash of (tensor, element): all 24 mantissa bits in use (the lowest is set), four binades, either sign
static float hashed(uint32_t tensor, uint32_t i) {
    uint32_t h = i * 0x9E3779B1u + tensor * 0x85EBCA77u + 0x165667B1u;
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    uint32_t u = (h & 0x80000000u) | ((124u + ((h >> 23) & 3u)) << 23) | (h & 0x007FFFFFu) | 1u;
    float f;
    memcpy(&f, &u, 4);
    return f;
}
struct Net {
    bb_net_weights w;
    std::vector<float> t[18]; // bb_net_weights' arrays in their order
};
static const char *tensor_names[18] = {"conv0_k", "conv0_b", "conv0_bn", "blk_k", "blk_b", "blk_bn", "v_conv_k", "v_conv_b", "v_bn",
                                       "v_d1_k", "v_d1_b", "v_d2_k", "v_d2_b", "p_conv_k", "p_conv_b", "p_bn", "p_d_k", "p_d_b"};
static void make_net(Net &n, int H, int W, int C, int A, int F, int R, int D) {
    const size_t size[18] = {(size_t)9 * C * F, (size_t)F, (size_t)4 * F, (size_t)R * 2 * 9 * F * F, (size_t)R * 2 * F, (size_t)R * 2 * 4 * F,
                             (size_t)F, 1, 4, (size_t)D, (size_t)D, (size_t)D, 1, (size_t)2 * F, 2, 8, (size_t)2 * A, (size_t)A};
    const int bn_filters[18] = {0, 0, F, 0, 0, F, 0, 0, 1, 0, 0, 0, 0, 0, 0, 2, 0, 0}; // [..][4][filters]: row 3 is the moving variance
    for (int k = 0; k < 18; k++) {
        n.t[k].resize(size[k]);
        for (size_t i = 0; i < size[k]; i++) {
            float v = hashed((uint32_t)k, (uint32_t)i);
            if (bn_filters[k] && (i / bn_filters[k]) % 4 == 3) v = v < 0 ? -v : v;
            n.t[k][i] = v;
        }
    }
    const float **field[18] = {&n.w.conv0_k, &n.w.conv0_b, &n.w.conv0_bn, &n.w.blk_k, &n.w.blk_b, &n.w.blk_bn, &n.w.v_conv_k, &n.w.v_conv_b,
                               &n.w.v_bn, &n.w.v_d1_k, &n.w.v_d1_b, &n.w.v_d2_k, &n.w.v_d2_b, &n.w.p_conv_k, &n.w.p_conv_b, &n.w.p_bn,
                               &n.w.p_d_k, &n.w.p_d_b};
    for (int k = 0; k < 18; k++) *field[k] = n.t[k].data();
    n.w.H = H; n.w.W = W; n.w.C = C; n.w.A = A; n.w.F = F; n.w.R = R; n.w.D = D;
}
static std::string g_dir, g_shape;
static void dump(const char *image, const void *p, size_t bytes) {
    std::string path = g_dir + "/" + g_shape + "." + image + ".bin";
    FILE *f = fopen(path.c_str(), "wb");
    if (!f || (bytes && fwrite(p, 1, bytes, f) != bytes)) { perror(path.c_str()); exit(2); }
    fclose(f);
}
template <class T> static void dump(const char *image, const std::vector<T> &v) { dump(image, v.data(), v.size() * sizeof(T)); }
static void pack_and_dump(const Net &n);   // every image of one network, to files
static double pack_as_a_load_does(const Net &n); // what one bb_load_weights packs in the default form; returns a checksum
// dump DIR name:H:W:C:A:F:R:D ...   |   time F R   (Connect4; prints the milliseconds of one packing, after one to warm up)
int main(int argc, char **argv) {
    if (argc >= 4 && !strcmp(argv[1], "time")) {
        Net n;
        make_net(n, 6, 7, 3, 7, atoi(argv[2]), atoi(argv[3]), 16);
        double sink = pack_as_a_load_does(n);
        auto t0 = std::chrono::steady_clock::now();
        sink += pack_as_a_load_does(n);
        auto t1 = std::chrono::steady_clock::now();
        printf("%.3f ms (checksum %.6g)\n", std::chrono::duration<double, std::milli>(t1 - t0).count(), sink);
        return 0;
    }
    if (argc < 3 || strcmp(argv[1], "dump")) return 2;
    g_dir = argv[2];
    for (int a = 3; a < argc; a++) {
        char name[64];
        int H, W, C, A, F, R, D;
        if (sscanf(argv[a], "%63[^:]:%d:%d:%d:%d:%d:%d:%d", name, &H, &W, &C, &A, &F, &R, &D) != 8) return 2;
        g_shape = name;
        Net n;
        make_net(n, H, W, C, A, F, R, D);
        for (int k = 0; k < 18; k++) dump((std::string("in_") + tensor_names[k]).c_str(), n.t[k]);
        pack_and_dump(n);
    }
    return 0;
}
"""

PROGRAM = '#include "net_pack.h"\n' + COMMON + r"""
static void pack_and_dump(const Net &n) {
    const bb_net_weights *w = &n.w;
    const NetF32 g = pack_f32(w, w->F / 16);
    dump("g_w0", g.w0);
    dump("g_wt", g.wt);
    dump("g_epi", g.epi);
    dump("g_x3", pack_gnet_x3(w, w->F / 16));
    const NetHead h = pack_head(w);
    const int off[11] = {h.off_vk, h.off_v3, h.off_d1k, h.off_d1b, h.off_d2k, h.off_d2b, h.off_pk, h.off_p6, h.off_pdk, h.off_pdb, (int)h.v.size()};
    dump("head", h.v);
    dump("head_off", off, sizeof off);
    if (w->F != 16) return;
    const NetF32 z(w->C, w->R, 1); // the sizes a wide network's unused fused operands get
    if (z.w0.size() != g.w0.size() || z.wt.size() != g.wt.size() || z.epi.size() != g.epi.size()) exit(3);
    const NetX3Image x = pack_x3(w);
    dump("x_w0", x.w0);
    dump("x_wt12", x.wt12);
    dump("x_wt3", x.wt3);
    dump("x_wt8", x.wt8);
    dump("x_wh", x.wh);
}
static double pack_as_a_load_does(const Net &n) {
    const bb_net_weights *w = &n.w;
    auto last = [](const auto &v) { return v.empty() ? 0.0 : (double)v.back(); };
    const NetF32 one = w->F == 16 ? pack_f32(w, 1) : NetF32(w->C, w->R, 1);
    const NetHead h = pack_head(w);
    double sum = last(one.w0) + last(one.wt) + last(one.epi) + last(h.v);
    if (w->F == 16) {
        const NetX3Image x = pack_x3(w);
        sum += last(x.w0) + last(x.wt12) + last(x.wt3) + last(x.wt8) + last(x.wh);
    } else {
        const NetF32 g = pack_f32(w, w->F / 16);
        sum += last(g.w0) + last(g.wt) + last(g.epi) + last(pack_gnet_x3(w, w->F / 16));
    }
    return sum;
}
"""

F32, U16, U32 = np.float32, np.uint16, np.uint32
SLICE_TAPS = np.array([[0, 1], [3, 4], [6, 7], [2, 5]])  # the four K = 32 slices of a tower layer; tap 8 goes alone


@pytest.fixture(scope="module")
def images(tmp_path_factory):
    """{shape: {image or in_<tensor>: bytes}} -- compiled, packed and read once for the module"""
    d = tmp_path_factory.mktemp("net_pack")
    src = d / "pack.cpp"
    src.write_text(PROGRAM)
    exe = d / "pack"
    subprocess.check_call([host_compiler(), "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-I", CSRC,
                           str(src), "-o", str(exe)])
    out = d / "out"
    out.mkdir()
    subprocess.check_call([str(exe), "dump", str(out)] + [":".join([k] + [str(x) for x in v]) for k, v in SHAPES.items()])
    res = {k: {} for k in SHAPES}
    for name in sorted(os.listdir(out)):
        shape, image, _ = name.split(".")
        res[shape][image] = (out / name).read_bytes()
    return res


def _same(a, b):
    """equal float32 arrays, bit for bit"""
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _split(x):
    """[3, *x.shape] uint16: plane k is the bf16 nearest (ties to even) to what planes < k leave of x"""
    x = np.ascontiguousarray(x, dtype=F32)
    p1 = _bf16_nearest(x)
    r = x - _widen(p1)
    p2 = _bf16_nearest(r)
    p3 = _bf16_nearest(r - _widen(p2))
    return np.stack([p1, p2, p3])


def _is_split_of(planes, x):
    """the three planes sum, smallest first, to x bit for bit -- and are THE split of x"""
    total = (_widen(planes[2]) + _widen(planes[1])) + _widen(planes[0])
    return _same(total, np.asarray(x, dtype=F32)) and np.array_equal(planes, _split(x))


def _tensors(img, C, A, F, R, D):
    t = {k: np.frombuffer(img["in_" + k], dtype=F32) for k in TENSORS}
    t["conv0_k"] = t["conv0_k"].reshape(9, C, F)         # [tap][channel][filter]
    t["blk_k"] = t["blk_k"].reshape(2 * R, 9, F, F)       # [layer][tap][channel][filter]
    t["p_conv_k"] = t["p_conv_k"].reshape(F, 2)
    return t


def _fold(bn):
    """[..., 4, n] gamma, beta, mean, variance -> scale, shift in float32, as the kernels' epilogue wants them"""
    g, b, m, v = (bn[..., k, :] for k in range(4))
    s = g / np.sqrt(v + F32(1e-3))
    return s, b - m * s


def _check_inputs(t):
    for k in ("conv0_bn", "blk_bn", "v_bn", "p_bn"):
        n = {"v_bn": 1, "p_bn": 2}.get(k, t["conv0_b"].size)
        assert (t[k].reshape(-1, 4, n)[:, 3] > 0).all(), k
    k = t["conv0_k"].ravel()
    assert (_bits(k) & 1).all() and len(set((_bits(k) >> 23) & 0xFF)) == 4  # 24-bit mantissas over four binades
    assert all((p != 0).mean() > 0.9 for p in _split(k))  # all three bf16 planes carry something
    assert _is_split_of(_split(k), k)


def _check_f32(img, t, C, F, R):
    NCB, steps0 = F // 16, (9 * C + 3) // 4
    # w0 [filter block][K step s][j][f]: row 4s + j of the [9C][F] kernel, filter 16 fb + f; rows past 9C are padding
    w0 = np.frombuffer(img["g_w0"], dtype=F32).reshape(NCB, steps0, 4, 16)
    rows = w0.transpose(1, 2, 0, 3).reshape(4 * steps0, F)
    assert _same(rows[:9 * C], t["conv0_k"].reshape(9 * C, F))
    assert not _bits(rows[9 * C:]).any()
    # wt [layer][filter block][channel block][tap][j][f][r]: channel 16 cb + 4j + r, filter 16 fb + f
    wt = np.frombuffer(img["g_wt"], dtype=F32).reshape(2 * R, NCB, NCB, 9, 4, 16, 4)
    assert _same(wt.transpose(0, 3, 2, 4, 6, 1, 5).reshape(2 * R, 9, F, F), t["blk_k"])
    # epi [layer, first convolution included][filter block][bias | scale | shift][16]
    epi = np.frombuffer(img["g_epi"], dtype=F32).reshape(1 + 2 * R, NCB, 3, 16).transpose(0, 2, 1, 3).reshape(1 + 2 * R, 3, F)
    bias = np.concatenate([t["conv0_b"].reshape(1, F), t["blk_b"].reshape(2 * R, F)])
    scale, shift = _fold(np.concatenate([t["conv0_bn"].reshape(1, 4, F), t["blk_bn"].reshape(2 * R, 4, F)]))
    assert _same(epi[:, 0], bias) and _same(epi[:, 1], scale) and _same(epi[:, 2], shift)


def _check_head(img, t):
    s1, t1 = _fold(t["v_bn"].reshape(4, 1))
    s2, t2 = _fold(t["p_bn"].reshape(4, 2))
    arrays = [t["v_conv_k"], np.concatenate([t["v_conv_b"], s1, t1]), t["v_d1_k"], t["v_d1_b"], t["v_d2_k"], t["v_d2_b"],
              t["p_conv_k"].ravel(), np.concatenate([t["p_conv_b"], s2, t2]), t["p_d_k"], t["p_d_b"]]
    head = np.frombuffer(img["head"], dtype=F32)
    off = np.frombuffer(img["head_off"], dtype=np.int32)
    at = 0
    for k, a in enumerate(arrays):  # back to back, each from a multiple of 4 floats on, zeros in between
        assert off[k] == at, k
        assert _same(head[at:at + a.size], a.astype(F32)), k
        end = at + (a.size + 3) // 4 * 4
        assert not _bits(head[at + a.size:end]).any(), k
        at = end
    assert off[10] == at == head.size


def _check_gnet_x3(img, t, F, R):
    NCB = F // 16
    blocks = np.frombuffer(img["g_x3"], dtype=U16).reshape(2 * R, NCB, NCB, 4 * 3 * 64 * 8 + 3 * 64 * 4)
    k = t["blk_k"].reshape(2 * R, 9, NCB, 16, NCB, 16)  # [layer][tap][cb][channel][fb][filter]
    # [layer][fb][cb] [slice][plane][tap of the slice][channel half][filter][8 channels]
    sl = blocks[..., :4 * 3 * 64 * 8].reshape(2 * R, NCB, NCB, 4, 3, 2, 2, 16, 8)
    want = k[:, SLICE_TAPS].reshape(2 * R, 4, 2, NCB, 2, 8, NCB, 16).transpose(0, 6, 3, 1, 2, 4, 7, 5)
    assert _is_split_of(sl.transpose(4, 0, 1, 2, 3, 5, 6, 7, 8), want)
    # then tap 8: [plane][lane group g][filter][4 channels]: channels 4g .. 4g + 3 of the block
    t8 = blocks[..., 4 * 3 * 64 * 8:].reshape(2 * R, NCB, NCB, 3, 4, 16, 4)
    want8 = k[:, 8].reshape(2 * R, NCB, 4, 4, NCB, 16).transpose(0, 4, 1, 2, 5, 3)
    assert _is_split_of(t8.transpose(3, 0, 1, 2, 4, 5, 6), want8)


def _check_x3(img, t, C, R):
    u16 = lambda name: np.frombuffer(img[name], dtype=U16)
    zero = lambda a: not np.asarray(a).any()
    # ---- first convolution
    w0 = u16("x_w0")
    if C <= 4:
        k0 = np.zeros((9, 4, 16), dtype=F32)
        k0[:, :C] = t["conv0_k"]
        # [plane][lane group g][filter][tap 2g or 2g + 1][4 input planes]: taps 0 .. 7
        taps = w0[:3 * 64 * 8].reshape(3, 4, 16, 2, 4).transpose(0, 1, 3, 4, 2).reshape(3, 8, 4, 16)
        assert _is_split_of(taps, k0[:8]) and zero(taps[:, :, C:])
        # tap 8 in ONE operand [lane group][filter][half][4 input planes]: group 0 = [w1 | w2], group 1 = [w3 | 0], groups 2, 3 unused
        op = w0[3 * 64 * 8:].reshape(4, 16, 2, 4)
        p = _split(k0[8]).transpose(0, 2, 1)  # [plane][filter][input plane]
        assert np.array_equal(op[0, :, 0], p[0]) and np.array_equal(op[0, :, 1], p[1]) and np.array_equal(op[1, :, 0], p[2])
        assert zero(op[1, :, 1]) and zero(op[2:]) and zero(op[..., C:])
    else:
        k0 = np.zeros((9, 32, 16), dtype=F32)
        k0[:, :C] = t["conv0_k"]
        # [tap][plane][lane group g][filter][8 input planes 8g ..]
        planes = w0.reshape(9, 3, 4, 16, 8).transpose(1, 0, 2, 4, 3).reshape(3, 9, 32, 16)
        assert _is_split_of(planes, k0) and zero(planes[:, :, C:])
    # ---- the head convolutions [operand][upper lane groups?][channel half][filter row][8 channels]; rows 0, 4, 8 = value, policy 0, policy 1
    wh = u16("x_wh").reshape(3, 2, 2, 16, 8)
    p = _split(np.stack([t["v_conv_k"], t["p_conv_k"][:, 0], t["p_conv_k"][:, 1]]).reshape(3, 2, 8)).transpose(0, 2, 1, 3)  # [plane][half][head][8]
    rows = wh[:, :, :, [0, 4, 8]]
    assert zero(np.delete(wh, [0, 4, 8], axis=3))
    for upper in (0, 1):  # the operands [w1|w1], [w2|w2], [w1|w3]: lane groups 2, 3 of the last hold plane 3
        assert np.array_equal(rows[0, upper], p[0]) and np.array_equal(rows[1, upper], p[1])
        assert np.array_equal(rows[2, upper], p[2 if upper else 0])
    # ---- tower layers: planes 1, 2 in wt12, plane 3 in wt3
    k = t["blk_k"]  # [layer][tap][channel][filter]
    wt12 = u16("x_wt12").reshape(2 * R, 4 * 2 * 64 * 8 + 2 * 32 * 8)
    wt3 = u16("x_wt3").reshape(2 * R, 4 * 64 * 8 + 64 * 8)
    # slices [slice][plane][tap of the slice][channel half][filter][8 channels]
    s12 = wt12[:, :4 * 2 * 64 * 8].reshape(2 * R, 4, 2, 2, 2, 16, 8).transpose(2, 0, 1, 3, 4, 5, 6)
    s3 = wt3[:, :4 * 64 * 8].reshape(1, 2 * R, 4, 2, 2, 16, 8)
    want = k[:, SLICE_TAPS].reshape(2 * R, 4, 2, 2, 8, 16).transpose(0, 1, 2, 3, 5, 4)
    assert _is_split_of(np.concatenate([s12, s3]), want)
    # tap 8, [layer][channel half][filter][8 channels], plane by plane
    p = _split(k[:, 8].reshape(2 * R, 2, 8, 16).transpose(0, 1, 3, 2))
    assert _is_split_of(p, k[:, 8].reshape(2 * R, 2, 8, 16).transpose(0, 1, 3, 2))
    t12 = wt12[:, 4 * 2 * 64 * 8:].reshape(2 * R, 2, 2, 16, 8)  # [plane][half][filter][8]
    assert np.array_equal(t12[:, 0], p[0]) and np.array_equal(t12[:, 1], p[1])
    t3 = wt3[:, 4 * 64 * 8:].reshape(2 * R, 2, 2, 16, 8)  # [w1 | w3]: lane groups 0, 1 plane 1; groups 2, 3 plane 3
    assert np.array_equal(t3[:, 0], p[0]) and np.array_equal(t3[:, 1], p[2])
    wt8 = u16("x_wt8").reshape(2 * R, 3, 2, 2, 16, 8)  # [w1|w1], [w2|w2], [w1|w3] as 64-lane images
    for upper in (0, 1):
        assert np.array_equal(wt8[:, 0, upper], p[0]) and np.array_equal(wt8[:, 1, upper], p[1])
        assert np.array_equal(wt8[:, 2, upper], p[2 if upper else 0])


@pytest.mark.parametrize("shape", list(SHAPES))
def test_images_unpack_to_the_weights(images, shape):
    H, W, C, A, F, R, D = SHAPES[shape]
    img = images[shape]
    t = _tensors(img, C, A, F, R, D)
    _check_inputs(t)
    _check_f32(img, t, C, F, R)
    _check_head(img, t)
    _check_gnet_x3(img, t, F, R)
    if F == 16:
        _check_x3(img, t, C, R)
    else:
        assert not any(k.startswith("x_") for k in img)


@pytest.mark.parametrize("shape", list(SHAPES))
def test_same_bytes_as_the_loops_inside_the_engine_gave(images, shape):
    """every image against the digests recorded from the former loops of engine.hip; at 16 filters those held the fused tower's
    operands (f_*) and the general network's (g_*) apart: the one packer at one block gives both"""
    with open(GOLDEN) as f:
        golden = json.load(f)[shape]
    img = images[shape]
    got = {k: hashlib.sha256(v).hexdigest() for k, v in img.items() if not k.startswith("in_")}
    got["inputs"] = hashlib.sha256(b"".join(img["in_" + k] for k in TENSORS)).hexdigest()
    if SHAPES[shape][4] == 16:
        for k in ("w0", "wt", "epi"):
            assert golden["f_" + k] == golden["g_" + k]
            got["f_" + k] = got["g_" + k]
    assert got == golden
