// avi_host.cpp -- MJPEG AVI demux (see avi_host.hpp).  Host only: no HIP, no other unit of the library.
#include "avi_host.hpp"

#include <exception>

namespace aeon_hip {

namespace {

constexpr uint32_t fourcc(char a, char b, char c, char d)
{
    return (uint32_t)(uint8_t)a | ((uint32_t)(uint8_t)b << 8) | ((uint32_t)(uint8_t)c << 16) | ((uint32_t)(uint8_t)d << 24);
}
constexpr uint32_t RIFF_CC = fourcc('R', 'I', 'F', 'F'), LIST_CC = fourcc('L', 'I', 'S', 'T');
constexpr uint32_t HDRL_CC = fourcc('h', 'd', 'r', 'l'), AVIH_CC = fourcc('a', 'v', 'i', 'h');
constexpr uint32_t STRL_CC = fourcc('s', 't', 'r', 'l'), STRH_CC = fourcc('s', 't', 'r', 'h');
constexpr uint32_t VIDS_CC = fourcc('v', 'i', 'd', 's'), MJPG_CC = fourcc('M', 'J', 'P', 'G');
constexpr uint32_t MOVI_CC = fourcc('m', 'o', 'v', 'i'), IDX1_CC = fourcc('i', 'd', 'x', '1');
constexpr uint32_t AVI_CC = fourcc('A', 'V', 'I', ' '), AVIX_CC = fourcc('A', 'V', 'I', 'X');
constexpr uint32_t JUNK_CC = fourcc('J', 'U', 'N', 'K'), INFO_CC = fourcc('I', 'N', 'F', 'O');

// aeon's std::istream over the datum: a position, and a failure that sticks (a read past the end sets
// failbit, after which every seekg and read of aeon's parse does nothing: the parse ends there)
struct span_reader {
    const uint8_t* data;
    uint64_t       size, pos = 0;
    bool           ok = true;
    void seek(uint64_t p)
    {
        if (ok) pos = p;
    }
    // n bytes at pos as little-endian dwords into out[0 .. n/4)
    bool dwords(uint32_t* out, int n)
    {
        if (!ok || pos > size || size - pos < (uint64_t)n) return ok = false;
        for (int i = 0; i < n / 4; i++) {
            const uint8_t* p = data + pos + 4 * (uint64_t)i;
            out[i]           = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
        }
        pos += (uint64_t)n;
        return true;
    }
};

struct riff_chunk { // avi.hpp:89-93
    uint32_t four_cc = 0, size = 0;
};
struct riff_list { // avi.hpp:95-100
    uint32_t riff_or_list_cc = 0, size = 0, list_type_cc = 0;
};
bool read(span_reader& in, riff_chunk& c)
{
    uint32_t v[2];
    if (!in.dwords(v, 8)) return false;
    c.four_cc = v[0], c.size = v[1];
    return true;
}
bool read(span_reader& in, riff_list& l)
{
    uint32_t v[3];
    if (!in.dwords(v, 12)) return false;
    l.riff_or_list_cc = v[0], l.size = v[1], l.list_type_cc = v[2];
    return true;
}
// RiffList::m_size includes the list type fourcc already read: aeon's uint32 (m_size - 4)
uint64_t list_rest(const riff_list& l) { return (uint64_t)(uint32_t)(l.size - 4u); }

enum reason { R_NONE, R_NOT_AVI, R_NO_MJPG, R_NOT_VALID, R_PAST, R_EMPTY_FIRST };

struct demux {
    span_reader     in;
    aeon_avi_frame* frames;
    int             cap;
    int64_t         count = 0; // index entries that are frames, kept or not
    uint32_t        width = 0, height = 0;
    reason          why = R_NONE;
    int64_t         bad_frame = -1;

    // one AVI / AVIX list with its own AviMjpegStream (cap_mjpeg_decoder.cpp:206)
    struct stream {
        uint32_t stream_id = 0, width = 0, height = 0;
        bool     index_present = false;
        uint64_t movi_start = 0, movi_end = 0;
    };

    // MotionJpegCapture::readFrame (cap_mjpeg_decoder.cpp:97-112) of a kept frame: the chunk header at
    // the index's position gives the size.  aeon reads past the datum here; this refuses.
    bool keep(uint64_t abs_pos)
    {
        if (count < cap) {
            const uint64_t size = in.size;
            if (abs_pos > size || size - abs_pos < 8) return why = R_PAST, bad_frame = count, false;
            const uint8_t* p  = in.data + abs_pos + 4;
            const uint32_t sz = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
            if (size - abs_pos - 8 < (uint64_t)sz) return why = R_PAST, bad_frame = count, false;
            // retrieveFrame keeps the previous iteration's cv::Mat for an empty chunk
            // (cap_mjpeg_decoder.cpp:138-141); before the first frame there is none
            if (count == 0 && sz == 0) return why = R_EMPTY_FIRST, false;
            frames[count] = aeon_avi_frame{abs_pos + 8, sz};
        }
        count++;
        return true;
    }

    // avi.cpp:145-177
    bool parse_index(const stream& s, uint32_t index_size)
    {
        const uint64_t index_end = in.pos + index_size;
        while (in.ok && in.pos < index_end) {
            uint32_t idx[4]; // AviIndex: ckid, dwFlags, dwChunkOffset, dwChunkLength
            if (!in.dwords(idx, 16)) break;
            if (idx[0] != s.stream_id) continue;
            const uint64_t abs_pos = s.movi_start + idx[2];
            if (abs_pos < s.movi_end && !keep(abs_pos)) return false;
        }
        return true;
    }

    // avi.cpp:179-217
    bool parse_strl(stream& s, uint8_t stream_index)
    {
        riff_chunk strh;
        if (!read(in, strh) || strh.four_cc != STRH_CC) return false;
        uint32_t hdr[14]; // AviStreamHeader (56 bytes): fccType, fccHandler, ...
        if (!in.dwords(hdr, 56)) return false;
        if (hdr[0] != VIDS_CC || hdr[1] != MJPG_CC) return false;
        if (s.stream_id == 0) // a second MJPG stream of the list is ignored
            s.stream_id = fourcc((char)(stream_index / 10 + '0'), (char)(stream_index % 10 + '0'), 'd', 'c');
        return true;
    }

    // avi.cpp:238-289
    bool parse_hdrl(stream& s)
    {
        riff_chunk avih;
        if (!read(in, avih) || avih.four_cc != AVIH_CC) return false;
        uint64_t next_strl = in.pos + avih.size;
        uint32_t hdr[14]; // AviMainHeader (56 bytes): [3] dwFlags, [6] dwStreams, [8] dwWidth, [9] dwHeight
        if (!in.dwords(hdr, 56)) return false;
        s.index_present = (hdr[3] & 0x10) != 0;
        s.width = hdr[8], s.height = hdr[9];
        bool result = false;
        for (uint32_t i = 0; i < hdr[6]; i++) {
            in.seek(next_strl);
            riff_list strl;
            // aeon goes on to the next stream after a list that is no strl; it would seek to the same
            // position and read the same bytes dwStreams times: one look is enough
            if (!read(in, strl) || strl.riff_or_list_cc != LIST_CC || strl.list_type_cc != STRL_CC) break;
            next_strl = in.pos + list_rest(strl);
            result    = parse_strl(s, (uint8_t)i);
        }
        if (!result && why == R_NONE) why = R_NO_MJPG;
        return result;
    }

    // avi.cpp:291-379; false: a refusal (why), not merely "no frames"
    bool parse_avi(stream& s)
    {
        riff_list hdrl;
        if (!read(in, hdrl) || hdrl.riff_or_list_cc != LIST_CC || hdrl.list_type_cc != HDRL_CC) return true;
        uint64_t next_list = in.pos + list_rest(hdrl);
        if (!parse_hdrl(s)) return true;
        in.seek(next_list);
        riff_list some;
        bool      got = read(in, some);
        if (got && some.riff_or_list_cc == LIST_CC && some.list_type_cc == INFO_CC) { // an optional INFO list
            next_list = in.pos + list_rest(some);
            in.seek(next_list);
            got = read(in, some);
        }
        if (got && some.riff_or_list_cc == JUNK_CC) { // an optional JUNK, read as a list header: size - 4 left
            in.seek(in.pos + list_rest(some));
            got = read(in, some);
        }
        if (!got || some.riff_or_list_cc != LIST_CC || some.list_type_cc != MOVI_CC) return true;
        s.movi_start = in.pos - 4; // the position of the movi fourcc
        s.movi_end   = s.movi_start + some.size;
        if (!s.index_present) return true; // without an index there are no frames (parseMovi is empty)
        in.seek(s.movi_start + 4 + list_rest(some));
        riff_chunk idx1;
        if (!read(in, idx1) || idx1.four_cc != IDX1_CC) return true;
        return parse_index(s, idx1.size);
    }

    // cap_mjpeg_decoder.cpp:190-227
    bool parse_riff()
    {
        bool first = true;
        while (in.ok) {
            riff_list riff;
            if (!read(in, riff) || riff.riff_or_list_cc != RIFF_CC ||
                !(riff.list_type_cc == AVI_CC || riff.list_type_cc == AVIX_CC)) {
                if (first) why = R_NOT_AVI;
                break;
            }
            first                    = false;
            const uint64_t next_riff = in.pos + list_rest(riff);
            stream         s;
            if (!parse_avi(s)) return false;
            if (count > 0) width = s.width, height = s.height; // parseAvi's result: the shared list has frames
            in.seek(next_riff);
        }
        return true;
    }
};

} // namespace

int avi_frames(const uint8_t* data, size_t size, aeon_avi_frame* frames, int cap, int* count, int* width, int* height,
               std::string& err)
{
    if (!count || cap < 0 || (cap > 0 && !frames) || (size > 0 && !data)) {
        err = "null argument";
        return AEON_HIP_EINVAL;
    }
    demux d{span_reader{data, (uint64_t)size}, frames, cap};
    const bool parsed = d.parse_riff();
    if (parsed && d.count > 0) {
        if (d.count > INT32_MAX) {
            err = "avi: too many frames";
            return AEON_HIP_EINVAL;
        }
        *count = (int)d.count;
        if (width) *width = (int)d.width;
        if (height) *height = (int)d.height;
        return AEON_HIP_OK;
    }
    switch (d.why) {
    case R_NOT_AVI: err = "avi: not a RIFF AVI file"; break;
    case R_PAST: err = "avi: the chunk of frame " + std::to_string(d.bad_frame) + " runs past the datum"; break;
    case R_EMPTY_FIRST: err = "avi: the first frame is empty"; break;
    case R_NO_MJPG: err = "avi: no MJPG video stream"; break;
    default: err = "Not a valid AVI file type"; break; // MotionJpegCapture::open: no index, no idx1, no frames
    }
    return AEON_HIP_EINVAL;
}

} // namespace aeon_hip

namespace {
thread_local std::string g_avi_err;
}

extern "C" {

int aeon_avi_frames(const void* data, size_t size, aeon_avi_frame* frames, int cap, int* count, int* width, int* height)
{
    try {
        return aeon_hip::avi_frames((const uint8_t*)data, size, frames, cap, count, width, height, g_avi_err);
    } catch (const std::exception& e) { // (std::string allocation)
        g_avi_err = e.what();
        return AEON_HIP_ERUNTIME;
    }
}

const char* aeon_avi_last_error(void) { return g_avi_err.c_str(); }

} // extern "C"
