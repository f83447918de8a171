// The walk over a BAM record's aux block by type, shared by the record writers that keep, drop or
// add tags (bsdc_zipper.hip, bsdc_group.hip).  Plain C++ with BSDC_HD: it compiles under g++ too.
// Everything here is inline: each including file has its own copy.
#ifndef BSDC_AUXWALK_H
#define BSDC_AUXWALK_H
#include <stdint.h>

#include <string>

#include "bsdc_devtext.h"

namespace bsdc_devtext {

// the value bytes of a fixed-size aux type, 0 for any other
BSDC_HD int zp_fixed(uint8_t t) {
    switch (t) {
    case 'A': case 'c': case 'C': return 1;
    case 's': case 'S': return 2;
    case 'i': case 'I': case 'f': return 4;
    default: return 0;
    }
}
// the end of the tag at a[i] in an aux block of n bytes; -1: an unknown type or a tag that leaves the block
BSDC_HD int64_t zp_tag_end(const uint8_t *a, int64_t i, int64_t n) {
    if (i + 3 > n) return -1;
    const uint8_t t = a[i + 2];
    int64_t j;
    if (const int f = zp_fixed(t)) {
        j = i + 3 + f;
    } else if (t == 'Z' || t == 'H') {
        j = i + 3;
        while (j < n && a[j]) j++;
        if (j >= n) return -1;
        j++;
    } else if (t == 'B') {
        if (i + 8 > n) return -1;
        const int es = a[i + 3] == 'A' ? 0 : zp_fixed(a[i + 3]);
        if (!es) return -1;
        const uint32_t cnt = (uint32_t)a[i + 4] | (uint32_t)a[i + 5] << 8 | (uint32_t)a[i + 6] << 16 | (uint32_t)a[i + 7] << 24;
        j = i + 8 + (int64_t)es * (int64_t)cnt;
    } else {
        return -1;
    }
    return j <= n ? j : -1;
}

// the read name of the record at r (its block_size field), "?" when it leaves the record
inline std::string zp_name(const uint8_t *r, int64_t rn) {
    const int l = r[12];
    return l >= 1 && 36 + l <= rn ? std::string((const char *)r + 36, (size_t)l - 1) : std::string("?");
}

// the first malformed tag of an aux block -> its description, "" when the block is well-formed
inline std::string zp_aux_error(const uint8_t *a, int64_t n) {
    for (int64_t i = 0; i < n;) {
        const int64_t j = zp_tag_end(a, i, n);
        if (j < 0) {
            if (i + 3 > n) return "trailing aux bytes";
            const uint8_t t = a[i + 2];
            const bool known = zp_fixed(t) || t == 'Z' || t == 'H' || (t == 'B' && i + 4 <= n && a[i + 3] != 'A' && zp_fixed(a[i + 3]));
            return std::string("aux tag ") + (char)a[i] + (char)a[i + 1] + (known ? " runs past the record" : " has an unknown type");
        }
        i = j;
    }
    return "";
}

}  // namespace bsdc_devtext
#endif
