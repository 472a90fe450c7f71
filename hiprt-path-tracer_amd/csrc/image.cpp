// image.cpp -- host-side PNG scanline reconstruction for the glTF texture loader
// (mpt/image.py).  The reference decodes textures with stb_image (Image8Bit::read_image,
// Image.cpp:33-61, called by ThreadFunctions::load_scene_texture, ThreadFunctions.cpp:30-97);
// the loader restates the PNG part of it: zlib inflate in Python's zlib, the per-row filter
// reversal here (sequential along a row: Python would take seconds on a 4K texture).
// Below it, the PNG writer of the screenshots (mpt_write_png).
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mpt.h"

namespace mpt {
int api_fail(int code, const char* msg);   // mpt_api.cpp: sets mpt_last_error
}

extern "C" int mpt_png_unfilter(const uint8_t* filtered, int64_t filtered_size, uint8_t* out, int32_t rows,
                                int32_t row_bytes, int32_t bpp) {
    if (!filtered || (!out && rows > 0)) return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (rows < 0 || row_bytes < 0 || bpp < 1 || bpp > 8)
        return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, "png: bad geometry");
    if (filtered_size < (int64_t)rows * (row_bytes + 1)) return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, "png: truncated image data");
    const uint8_t* prev = nullptr;
    for (int32_t y = 0; y < rows; y++) {
        const uint8_t* src = filtered + (size_t)y * (row_bytes + 1);
        uint8_t* dst = out + (size_t)y * row_bytes;
        const int type = src[0];
        src++;
        switch (type) {
        case 0:   // None
            std::memcpy(dst, src, (size_t)row_bytes);
            break;
        case 1:   // Sub
            for (int32_t i = 0; i < row_bytes; i++) dst[i] = (uint8_t)(src[i] + (i >= bpp ? dst[i - bpp] : 0));
            break;
        case 2:   // Up
            for (int32_t i = 0; i < row_bytes; i++) dst[i] = (uint8_t)(src[i] + (prev ? prev[i] : 0));
            break;
        case 3:   // Average
            for (int32_t i = 0; i < row_bytes; i++) {
                const int a = i >= bpp ? dst[i - bpp] : 0, b = prev ? prev[i] : 0;
                dst[i] = (uint8_t)(src[i] + ((a + b) >> 1));
            }
            break;
        case 4:   // Paeth
            for (int32_t i = 0; i < row_bytes; i++) {
                const int a = i >= bpp ? dst[i - bpp] : 0, b = prev ? prev[i] : 0;
                const int c = (i >= bpp && prev) ? prev[i - bpp] : 0;
                const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
                const int pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
                dst[i] = (uint8_t)(src[i] + pred);
            }
            break;
        default:
            return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, "png: bad filter type");
        }
        prev = dst;
    }
    return MPT_OK;
}

// ---------------------------------------------------------------------------------------
// PNG writer of the screenshots (the reference calls stbi_write_png, Screenshoter.cpp:162-163):
// 8-bit RGBA, filter type None on every scanline, the zlib stream made of stored (uncompressed)
// deflate blocks of up to 65535 bytes -- any decoder reads it, and nothing is linked for it.
// ---------------------------------------------------------------------------------------
namespace {

struct Crc32Table {
    uint32_t t[256];
    Crc32Table() {
        for (uint32_t n = 0; n < 256; n++) {
            uint32_t c = n;
            for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
            t[n] = c;
        }
    }
};

uint32_t crc32(uint32_t crc, const uint8_t* p, size_t n) {
    static const Crc32Table table;
    crc = ~crc;
    for (size_t i = 0; i < n; i++) crc = table.t[(crc ^ p[i]) & 0xffu] ^ (crc >> 8);
    return ~crc;
}

void put_be32(std::vector<uint8_t>& v, uint32_t x) {
    v.push_back((uint8_t)(x >> 24)); v.push_back((uint8_t)(x >> 16)); v.push_back((uint8_t)(x >> 8)); v.push_back((uint8_t)x);
}

// one chunk: length, type, data, CRC-32 of type + data
bool write_chunk(FILE* f, const char type[4], const uint8_t* data, size_t n) {
    std::vector<uint8_t> head;
    put_be32(head, (uint32_t)n);
    head.insert(head.end(), type, type + 4);
    uint32_t crc = crc32(0u, head.data() + 4, 4);
    crc = crc32(crc, data, n);
    std::vector<uint8_t> tail;
    put_be32(tail, crc);
    return fwrite(head.data(), 1, 8, f) == 8 && (n == 0 || fwrite(data, 1, n, f) == n) && fwrite(tail.data(), 1, 4, f) == 4;
}

}  // namespace

extern "C" int mpt_write_png(const char* path, const uint8_t* rgba8, int32_t width, int32_t height, int32_t flip_y) {
    if (!path || !rgba8) return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, "NULL argument");
    if (width <= 0 || height <= 0) return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, "png: bad size");
    const size_t row = (size_t)width * 4, raw_n = (size_t)height * (row + 1);
    // the zlib stream: header, stored blocks (BFINAL, LEN, ~LEN little-endian, the bytes), Adler-32
    std::vector<uint8_t> z;
    z.reserve(raw_n + 5 * (raw_n / 65535 + 1) + 6);
    z.push_back(0x78); z.push_back(0x01);
    std::vector<uint8_t> raw(raw_n);
    for (int32_t y = 0; y < height; y++) {
        uint8_t* d = raw.data() + (size_t)y * (row + 1);
        d[0] = 0;   // filter type None
        std::memcpy(d + 1, rgba8 + (size_t)(flip_y ? height - 1 - y : y) * row, row);
    }
    uint32_t a = 1, b = 0;   // Adler-32, reduced often enough that b cannot overflow
    for (size_t i = 0; i < raw_n;) {
        const size_t n = raw_n - i < 5552 ? raw_n - i : 5552;
        for (size_t k = 0; k < n; k++) { a += raw[i + k]; b += a; }
        a %= 65521u; b %= 65521u;
        i += n;
    }
    for (size_t i = 0; i < raw_n;) {
        const size_t n = raw_n - i < 65535 ? raw_n - i : 65535;
        z.push_back(i + n == raw_n ? 1 : 0);
        z.push_back((uint8_t)(n & 0xff)); z.push_back((uint8_t)(n >> 8));
        z.push_back((uint8_t)(~n & 0xff)); z.push_back((uint8_t)((~n >> 8) & 0xff));
        z.insert(z.end(), raw.begin() + (ptrdiff_t)i, raw.begin() + (ptrdiff_t)(i + n));
        i += n;
    }
    put_be32(z, (b << 16) | a);
    FILE* f = fopen(path, "wb");
    if (!f) return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, "png: cannot open the file for writing");
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    std::vector<uint8_t> ihdr;
    put_be32(ihdr, (uint32_t)width);
    put_be32(ihdr, (uint32_t)height);
    const uint8_t fmt[5] = {8, 6, 0, 0, 0};   // 8 bits, RGBA, deflate, adaptive filtering, no interlace
    ihdr.insert(ihdr.end(), fmt, fmt + 5);
    bool ok = fwrite(sig, 1, 8, f) == 8 && write_chunk(f, "IHDR", ihdr.data(), ihdr.size());
    const size_t IDAT_MAX = (size_t)1 << 30;   // a chunk's length is 31 bits
    for (size_t i = 0; ok && i < z.size(); i += IDAT_MAX)
        ok = write_chunk(f, "IDAT", z.data() + i, z.size() - i < IDAT_MAX ? z.size() - i : IDAT_MAX);
    ok = ok && write_chunk(f, "IEND", nullptr, 0);
    ok = (fclose(f) == 0) && ok;
    if (!ok) return mpt::api_fail(MPT_ERR_INVALID_ARGUMENT, "png: write failed");
    return MPT_OK;
}
