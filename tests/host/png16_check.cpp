// png16_check.cpp -- the PNG reader (csrc/uva_pngread.cpp) run alone on 16-bit files, without HIP and without a GPU, so that it
// can be built with -fsanitize=address,undefined (tests/test_png16_sanitized.py).  The files are made here: 16-bit RGB, RGBA and
// grey (and 8-bit RGB) images, all five filter types, as a stored deflate stream or as fixed-Huffman literals.  Each must decode
// to its pixels; then a few hundred mutants of them -- one byte changed, with the chunk CRCs left wrong or made right again so
// that the damage reaches the inflate and the un-filter, and truncations -- go through the reader into a buffer of exactly the
// size it asked for.  A mutant may decode or be refused; it may not make the reader touch memory it does not own.  Prints one
// line of counts; the first violation ends the run with exit status 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

namespace uva {
int png_read_bgr16(const uint8_t* file, size_t len, uint16_t* out, size_t cap, int* h_out, int* w_out, std::string& err);
int png_read_bgr(const uint8_t* file, size_t len, uint8_t* out, size_t cap, int* h_out, int* w_out, std::string& err);
}

namespace {

typedef std::vector<uint8_t> Bytes;

[[noreturn]] void violation(const std::string& what)
{
    std::fprintf(stderr, "png16_check: %s\n", what.c_str());
    std::exit(1);
}

uint32_t crc32(const uint8_t* p, size_t n)
{
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; ++i) {
        c ^= p[i];
        for (int k = 0; k < 8; ++k) c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
    }
    return ~c;
}

uint32_t adler32(const Bytes& d)
{
    uint32_t a = 1, b = 0;
    for (uint8_t v : d) { a = (a + v) % 65521; b = (b + a) % 65521; }
    return a | (b << 16);
}

void be32(Bytes& o, uint32_t v) { for (int s = 24; s >= 0; s -= 8) o.push_back((uint8_t)(v >> s)); }

void chunk(Bytes& o, const char* tag, const Bytes& body)
{
    be32(o, (uint32_t)body.size());
    const size_t at = o.size();
    o.insert(o.end(), tag, tag + 4);
    o.insert(o.end(), body.begin(), body.end());
    be32(o, crc32(o.data() + at, 4 + body.size()));
}

struct BitWriter {
    Bytes bytes;
    int nbits = 0;
    void put(uint32_t v, int n)                       // LSB first
    {
        for (int i = 0; i < n; ++i, ++nbits) {
            if ((nbits & 7) == 0) bytes.push_back(0);
            bytes.back() |= (uint8_t)(((v >> i) & 1u) << (nbits & 7));
        }
    }
    void code(uint32_t v, int n) { for (int i = n - 1; i >= 0; --i) put((v >> i) & 1u, 1); }     // Huffman codes: MSB first
};

// zlib stream of `raw`: stored blocks of at most 40 000 bytes, or one fixed-Huffman block of literals (RFC 1951 3.2.6)
Bytes deflate(const Bytes& raw, bool huffman)
{
    Bytes z = {0x78, 0x01};
    if (huffman) {
        BitWriter w;
        w.put(1, 1); w.put(1, 2);
        for (uint8_t v : raw) {
            if (v < 144) w.code(0x30 + v, 8);
            else w.code(0x190 + (v - 144), 9);
        }
        w.code(0, 7);
        z.insert(z.end(), w.bytes.begin(), w.bytes.end());
    } else {
        size_t pos = 0;
        do {
            const size_t n = std::min<size_t>(40000, raw.size() - pos);
            z.push_back(pos + n == raw.size() ? 1 : 0);
            z.push_back((uint8_t)n); z.push_back((uint8_t)(n >> 8));
            z.push_back((uint8_t)~n); z.push_back((uint8_t)(~n >> 8));
            z.insert(z.end(), raw.begin() + pos, raw.begin() + pos + n);
            pos += n;
        } while (pos < raw.size());
    }
    be32(z, adler32(raw));
    return z;
}

int paeth(int a, int b, int c)
{
    const int p = a + b - c, pa = std::abs(p - a), pb = std::abs(p - b), pc = std::abs(p - c);
    return (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
}

struct Image {
    int h, w, channels, depth;
    std::vector<uint16_t> pix;         // [h][w][channels], file order (R G B A / grey)
    Bytes file;
};

Image make(int h, int w, int channels, int depth, bool huffman, std::mt19937& rng)
{
    Image im{h, w, channels, depth, {}, {}};
    im.pix.resize((size_t)h * w * channels);
    for (auto& v : im.pix) v = (uint16_t)(depth == 16 ? rng() & 0xffff : rng() & 0xff);
    const int bps = depth / 8, bpp = channels * bps, rowb = w * bpp;
    Bytes lines((size_t)h * rowb), raw;
    for (size_t i = 0; i < im.pix.size(); ++i) {
        if (bps == 2) { lines[2 * i] = (uint8_t)(im.pix[i] >> 8); lines[2 * i + 1] = (uint8_t)im.pix[i]; }
        else lines[i] = (uint8_t)im.pix[i];
    }
    for (int y = 0; y < h; ++y) {
        const int ft = y % 5;
        raw.push_back((uint8_t)ft);
        for (int i = 0; i < rowb; ++i) {
            const int a = i >= bpp ? lines[(size_t)y * rowb + i - bpp] : 0, b = y ? lines[(size_t)(y - 1) * rowb + i] : 0;
            const int c = (i >= bpp && y) ? lines[(size_t)(y - 1) * rowb + i - bpp] : 0;
            const int pred = ft == 0 ? 0 : ft == 1 ? a : ft == 2 ? b : ft == 3 ? (a + b) / 2 : paeth(a, b, c);
            raw.push_back((uint8_t)(lines[(size_t)y * rowb + i] - pred));
        }
    }
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    im.file.assign(sig, sig + 8);
    Bytes ihdr;
    be32(ihdr, (uint32_t)w); be32(ihdr, (uint32_t)h);
    ihdr.push_back((uint8_t)depth);
    ihdr.push_back((uint8_t)(channels == 1 ? 0 : channels == 3 ? 2 : 6));
    ihdr.push_back(0); ihdr.push_back(0); ihdr.push_back(0);
    chunk(im.file, "IHDR", ihdr);
    const Bytes z = deflate(raw, huffman);
    const size_t half = z.size() / 2;                 // two IDAT chunks: the reader's concatenating path
    chunk(im.file, "IDAT", Bytes(z.begin(), z.begin() + half));
    chunk(im.file, "IDAT", Bytes(z.begin() + half, z.end()));
    chunk(im.file, "IEND", Bytes());
    return im;
}

// the reader as its callers drive it: size query, then a buffer of exactly that size (ASan watches its ends)
int decode(const Bytes& file, std::vector<uint16_t>& out, int* h, int* w)
{
    std::string err;
    *h = *w = 0;
    const Bytes copy(file);                            // (a heap block of exactly the file's length)
    int rc = uva::png_read_bgr16(copy.data(), copy.size(), nullptr, 0, h, w, err);
    if (rc) return rc;
    if (*h <= 0 || *w <= 0) violation("size query succeeded without a size");
    if ((size_t)*h * (size_t)*w > (1u << 22)) return 1;        // (a mutant's header may honestly claim more than the test wants to allocate)
    out.assign((size_t)*h * *w * 3, 0);
    rc = uva::png_read_bgr16(copy.data(), copy.size(), out.data(), out.size() * 2, h, w, err);
    if (rc == 1 && err.empty()) violation("refused without a message");
    return rc;
}

void fix_crcs(Bytes& f)
{
    size_t pos = 8;
    while (pos + 12 <= f.size()) {
        const size_t n = ((size_t)f[pos] << 24) | ((size_t)f[pos + 1] << 16) | ((size_t)f[pos + 2] << 8) | f[pos + 3];
        if (n > f.size() - pos - 12) return;
        const uint32_t c = crc32(f.data() + pos + 4, 4 + n);
        for (int k = 0; k < 4; ++k) f[pos + 8 + n + k] = (uint8_t)(c >> (24 - 8 * k));
        pos += 12 + n;
    }
}

}  // namespace

int main()
{
    std::mt19937 rng(16);
    std::vector<Image> images;
    images.push_back(make(1, 1, 3, 16, false, rng));
    images.push_back(make(9, 1, 3, 16, true, rng));
    images.push_back(make(1, 7, 4, 16, false, rng));
    images.push_back(make(37, 53, 3, 16, true, rng));
    images.push_back(make(11, 13, 1, 16, true, rng));
    images.push_back(make(12, 9, 4, 16, true, rng));
    images.push_back(make(90, 131, 3, 16, false, rng));       // two stored blocks
    images.push_back(make(10, 17, 3, 8, true, rng));          // an 8-bit file: widened v * 257
    long valid = 0, mutants = 0, decoded = 0, refused = 0, declined = 0;
    std::vector<uint16_t> out;
    int h, w;
    for (const Image& im : images) {
        if (decode(im.file, out, &h, &w) != 0) violation("a valid file was refused");
        if (h != im.h || w != im.w) violation("wrong size");
        for (int y = 0; y < h; ++y)
            for (int x = 0; x < w; ++x)
                for (int c = 0; c < 3; ++c) {
                    const uint16_t* p = &im.pix[((size_t)y * w + x) * im.channels];
                    uint16_t want = im.channels == 1 ? p[0] : p[2 - c];
                    if (im.depth == 8) want = (uint16_t)(want * 257);
                    if (out[((size_t)y * w + x) * 3 + c] != want) violation("wrong pixel");
                }
        ++valid;
        // the 8-bit entry on the same file: 16-bit files are declined (2), the 8-bit one decodes
        std::vector<uint8_t> out8((size_t)h * w * 3);
        std::string err;
        const int rc8 = uva::png_read_bgr(im.file.data(), im.file.size(), out8.data(), out8.size(), &h, &w, err);
        if (rc8 != (im.depth == 16 ? 2 : 0)) violation("the 8-bit reader's answer changed");
    }
    for (const Image& im : images) {
        for (int k = 0; k < 60; ++k) {
            Bytes f = im.file;
            const size_t at = k < 20 ? 8 + rng() % 40 % f.size() : rng() % f.size();        // the header region gets its share
            const uint8_t bit = (uint8_t)(1u << (rng() % 8));
            f[at] = (k % 3 == 0) ? (uint8_t)rng() : (uint8_t)(f[at] ^ bit);
            if (k % 2) fix_crcs(f);
            const int rc = decode(f, out, &h, &w);
            ++mutants;
            ++(rc == 0 ? decoded : rc == 1 ? refused : declined);
        }
        for (int k = 0; k < 12; ++k) {
            Bytes f(im.file.begin(), im.file.begin() + (k < 4 ? (size_t)k * 11 % im.file.size() : rng() % im.file.size()));
            if (decode(f, out, &h, &w) == 0) violation("a truncated file decoded");
            ++mutants; ++refused;
        }
    }
    std::printf("png16_check: %ld valid files, %ld mutants (%ld decoded, %ld refused, %ld declined): ok\n", valid, mutants, decoded, refused,
                declined);
    return 0;
}
