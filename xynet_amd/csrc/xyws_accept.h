// xyws_accept.h — internal: the opening handshake of one connection, stated
// once for the host and the device (include/xyws.h states the semantics):
// picohttpparser's request walk, the two policies' checks, SHA-1, base64 and
// the three responses. xyws_accept_streams' kernel (xyws_accept.hip) runs
// evaluate() over a request staged in LDS; xyws_accept_request is the same
// function over host memory. The header needs nothing of HIP: a plain C++
// compiler takes it as it is (tests/cpp/accept_host_check.cpp).
#pragma once
#include <stdint.h>

#include "xyws.h"

#if defined(__HIPCC__)
#define XYWS_HD __host__ __device__ inline __attribute__((always_inline))
#define XYWS_HD_UNROLL _Pragma("unroll")
#else
#define XYWS_HD inline
#define XYWS_HD_UNROLL
#endif

namespace xyws_accept {

constexpr uint32_t RESP_101_LEN = 129, RESP_101_KEY = 97;  // the accept value's position in the 101
constexpr uint32_t RESP_400_REF_LEN = 26, RESP_400_LEN = 66, RESP_426_LEN = 98;
constexpr uint32_t RESP_MAX = 144;  // the 101 up to a multiple of 16
constexpr uint32_t MAX_HEADERS = 100;
constexpr uint32_t NO_KEY = 0xFFFFFFFFu;
constexpr uint32_t POLICY_BITS = XYWS_ACC_REFERENCE;

// The refusals of both entry points that their common arguments decide.
XYWS_HD bool args_ok(uint32_t max_request, uint32_t policy) {
  return max_request != 0 && max_request <= XYWS_ACCEPT_MAX_REQUEST && !(policy & ~POLICY_BITS);
}

// Request bytes: b[i] for i < E only.
struct host_bytes {
  const uint8_t* p;
  XYWS_HD uint8_t operator[](uint32_t i) const { return p[i]; }
};

// ---------------------------------------------------------------- SHA-1, base64
XYWS_HD uint32_t rol32(uint32_t x, uint32_t n) { return (x << n) | (x >> (32u - n)); }

// One 64-byte block (w: its 16 big-endian words, overwritten).
XYWS_HD void sha1_block(uint32_t h[5], uint32_t w[16]) {
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
  XYWS_HD_UNROLL
  for (uint32_t t = 0; t < 80; t++) {
    if (t >= 16) w[t & 15] = rol32(w[(t + 13) & 15] ^ w[(t + 8) & 15] ^ w[(t + 2) & 15] ^ w[t & 15], 1);
    uint32_t f, k;
    if (t < 20) {
      f = (b & c) | (~b & d);
      k = 0x5A827999u;
    } else if (t < 40) {
      f = b ^ c ^ d;
      k = 0x6ED9EBA1u;
    } else if (t < 60) {
      f = (b & c) | (b & d) | (c & d);
      k = 0x8F1BBCDCu;
    } else {
      f = b ^ c ^ d;
      k = 0xCA62C1D6u;
    }
    const uint32_t x = rol32(a, 5) + f + e + k + w[t & 15];
    e = d;
    d = c;
    c = rol32(b, 30);
    b = a;
    a = x;
  }
  h[0] += a;
  h[1] += b;
  h[2] += c;
  h[3] += d;
  h[4] += e;
}

XYWS_HD uint8_t base64_char(uint32_t v) {
  return (uint8_t)(v < 26 ? 'A' + v : v < 52 ? 'a' + (v - 26) : v < 62 ? '0' + (v - 52) : v == 62 ? '+' : '/');
}

// The 28 characters of Sec-WebSocket-Accept for the 24 key bytes: the message
// is key + GUID, 60 bytes, so two blocks: the pad byte at 60, the length (480
// bits) at the end of the second.
// kw: the key as six big-endian words.
XYWS_HD void accept_value(const uint32_t kw[6], uint8_t* out) {
  const char* const guid = "258EAFA5-E914-47DA-95CA-C5AB0DC85B11";
  uint32_t w[16];
  XYWS_HD_UNROLL
  for (uint32_t i = 0; i < 6; i++) w[i] = kw[i];
  XYWS_HD_UNROLL
  for (uint32_t i = 0; i < 9; i++)
    w[6 + i] = ((uint32_t)(uint8_t)guid[4 * i] << 24) | ((uint32_t)(uint8_t)guid[4 * i + 1] << 16) |
               ((uint32_t)(uint8_t)guid[4 * i + 2] << 8) | (uint32_t)(uint8_t)guid[4 * i + 3];
  w[15] = 0x80000000u;
  uint32_t h[5] = {0x67452301u, 0xEFCDAB89u, 0x98BADCFEu, 0x10325476u, 0xC3D2E1F0u};
  sha1_block(h, w);
  for (uint32_t i = 0; i < 15; i++) w[i] = 0;
  w[15] = 480;
  sha1_block(h, w);
  // 20 digest bytes -> 6 groups of 3 and one of 2
  for (uint32_t g = 0; g < 7; g++) {
    uint32_t v = 0;
    for (uint32_t j = 0; j < 3; j++) {
      const uint32_t q = 3 * g + j;
      v = (v << 8) | (q < 20 ? (h[q >> 2] >> (24 - 8 * (q & 3))) & 0xFFu : 0u);
    }
    out[4 * g] = base64_char(v >> 18);
    out[4 * g + 1] = base64_char((v >> 12) & 63);
    out[4 * g + 2] = base64_char((v >> 6) & 63);
    out[4 * g + 3] = g < 6 ? base64_char(v & 63) : (uint8_t)'=';
  }
}

// ---------------------------------------------------------------- byte classes
XYWS_HD bool is_token_char(uint32_t c) {  // picohttpparser's token_char_map
  if ((c >= '0' && c <= '9') || (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z')) return true;
  switch (c) {
    case '!': case '#': case '$': case '%': case '&': case '\'': case '*': case '+': case '-': case '.':
    case '^': case '_': case '`': case '|': case '~':
      return true;
    default:
      return false;
  }
}
XYWS_HD uint32_t lower(uint32_t c) { return c >= 'A' && c <= 'Z' ? c + 32 : c; }
XYWS_HD bool is_base64_char(uint32_t c) {
  return (c >= '0' && c <= '9') || (c >= 'A' && c <= 'Z') || (c >= 'a' && c <= 'z') || c == '+' || c == '/';
}

// A name or value to compare with, at most 24 characters, packed into three
// words at compile time (XYWS_LIT): both sides compare against registers, not
// against characters loaded from memory one at a time (14 such loops in the
// kernel before; the host call went from 730 to 580 ns per request).
struct lit {
  uint64_t w0, w1, w2;
  uint32_t n;
};
constexpr lit make_lit(const char* s, uint32_t n) {
  lit L = {0, 0, 0, n};
  for (uint32_t i = 0; i < n; i++) {
    const uint64_t c = (uint64_t)(uint8_t)s[i] << (8u * (i & 7u));
    if (i < 8) L.w0 |= c;
    else if (i < 16) L.w1 |= c;
    else L.w2 |= c;
  }
  return L;
}
#define XYWS_LIT(s)                                                                \
  ([]() {                                                                          \
    static_assert(sizeof(s) - 1 <= 24, "three words");                             \
    constexpr ::xyws_accept::lit L_ = ::xyws_accept::make_lit(s, sizeof(s) - 1);   \
    return L_;                                                                     \
  }())
XYWS_HD uint32_t lit_char(lit L, uint32_t i) {
  const uint64_t w = i < 8 ? L.w0 : i < 16 ? L.w1 : L.w2;
  return (uint32_t)(w >> (8u * (i & 7u))) & 0xFFu;
}

// b[off, off + len) equal to L (ci: L is lower case, the bytes are compared in
// lower case).
template <class R>
XYWS_HD bool span_is(const R& b, uint32_t off, uint32_t len, lit L, bool ci) {
  if (len != L.n) return false;
  for (uint32_t i = 0; i < L.n; i++) {
    const uint32_t c = b[off + i];
    if ((ci ? lower(c) : c) != lit_char(L, i)) return false;
  }
  return true;
}

// Some comma-separated element of b[off, off + len), SP/HT trimmed, equal to
// L without regard to case.
template <class R>
XYWS_HD bool has_element(const R& b, uint32_t off, uint32_t len, lit L) {
  uint32_t s = off;
  const uint32_t end = off + len;
  for (;;) {
    uint32_t e = s;
    while (e < end && b[e] != ',') e++;
    uint32_t x = s, y = e;
    while (x < y && (b[x] == ' ' || b[x] == '\t')) x++;
    while (y > x && (b[y - 1] == ' ' || b[y - 1] == '\t')) y--;
    if (span_is(b, x, y - x, L, true)) return true;
    if (e >= end) return false;
    s = e + 1;
  }
}

// The canonical base64 of 16 bytes: 21 alphabet characters, one of AQgw, ==.
template <class R>
XYWS_HD bool key_is_canonical(const R& b, uint32_t off, uint32_t len) {
  if (len != 24) return false;
  for (uint32_t i = 0; i < 21; i++)
    if (!is_base64_char(b[off + i])) return false;
  const uint32_t c = b[off + 21];
  return (c == 'A' || c == 'Q' || c == 'g' || c == 'w') && b[off + 22] == '=' && b[off + 23] == '=';
}

// ---------------------------------------------------------------- the walk and the checks
struct verdict {
  uint32_t status, http_status, reason, consumed, resp_len, path_off, path_len, key_off;
};

// What the headers seen so far say under each policy: a header is checked
// when the walk has its value, so no header table is kept; a walk that ends
// in an error or at the end of the bytes drops it all.
struct checks {
  uint32_t fail = 0;  // bit r: check XYWS_ACR_r failed
  uint32_t key_off = NO_KEY;
  uint32_t keys = 0, versions = 0;
  bool folded = false, host = false, upgrade = false, connection = false;
};

template <class R>
XYWS_HD void check_header(const R& b, bool ref, checks& k, bool named, uint32_t n0, uint32_t nl, uint32_t v0,
                          uint32_t vl) {
  if (ref) {
    // http_parser::headers() ends at the first nameless header
    if (!named) k.folded = true;
    if (k.folded) return;
    if (span_is(b, n0, nl, XYWS_LIT("Connection"), false)) {
      if (!span_is(b, v0, vl, XYWS_LIT("Upgrade"), false)) k.fail |= 1u << XYWS_ACR_CONNECTION;
    } else if (span_is(b, n0, nl, XYWS_LIT("Upgrade"), false)) {
      if (!span_is(b, v0, vl, XYWS_LIT("websocket"), false)) k.fail |= 1u << XYWS_ACR_UPGRADE;
    } else if (span_is(b, n0, nl, XYWS_LIT("Sec-WebSocket-Version"), false)) {
      if (!span_is(b, v0, vl, XYWS_LIT("13"), false)) k.fail |= 1u << XYWS_ACR_WS_VERSION;
    } else if (span_is(b, n0, nl, XYWS_LIT("Sec-WebSocket-Key"), false)) {
      if (vl == 24) k.key_off = v0;
      else k.fail |= 1u << XYWS_ACR_KEY;
    }
    return;
  }
  if (!named) {
    k.fail |= 1u << XYWS_ACR_FOLDED;
    return;
  }
  if (span_is(b, n0, nl, XYWS_LIT("host"), true)) {
    k.host = true;
  } else if (span_is(b, n0, nl, XYWS_LIT("upgrade"), true)) {
    if (has_element(b, v0, vl, XYWS_LIT("websocket"))) k.upgrade = true;
  } else if (span_is(b, n0, nl, XYWS_LIT("connection"), true)) {
    if (has_element(b, v0, vl, XYWS_LIT("upgrade"))) k.connection = true;
  } else if (span_is(b, n0, nl, XYWS_LIT("sec-websocket-key"), true)) {
    k.keys++;
    if (key_is_canonical(b, v0, vl)) k.key_off = v0;
    else k.fail |= 1u << XYWS_ACR_KEY;
  } else if (span_is(b, n0, nl, XYWS_LIT("sec-websocket-version"), true)) {
    k.versions++;
    if (!span_is(b, v0, vl, XYWS_LIT("13"), false)) k.fail |= 1u << XYWS_ACR_WS_VERSION;
  }
}

enum { EV_PARSED = 0, EV_ERROR = -1, EV_INCOMPLETE = -2 };

struct request {
  uint32_t consumed, method_off, method_len, path_off, path_len, minor;
};

// phr_parse_request's walk over b[0, E) (picohttpparser.h:426-494 with
// last_len == 0), each header handed to check_header as it ends.
template <class R>
XYWS_HD int walk(const R& b, uint32_t E, bool ref, request& rq, checks& k) {
  uint32_t p = 0;
  if (p == E) return EV_INCOMPLETE;
  if (b[p] == '\r') {  // one leading empty line
    p++;
    if (p == E) return EV_INCOMPLETE;
    if (b[p++] != '\n') return EV_ERROR;
  } else if (b[p] == '\n') {
    p++;
  }
  uint32_t tok[2][2];
  for (uint32_t i = 0; i < 2; i++) {  // method, target
    const uint32_t t0 = p;
    for (;;) {
      if (p == E) return EV_INCOMPLETE;
      const uint32_t c = b[p];
      if (c == ' ') break;
      if (c < 0x20 || c == 0x7f) return EV_ERROR;
      p++;
    }
    tok[i][0] = t0;
    tok[i][1] = p - t0;
    do p++;
    while (p < E && b[p] == ' ');  // (the end of the bytes is not a space)
  }
  if (tok[0][1] == 0 || tok[1][1] == 0) return EV_ERROR;
  if (E - p < 9) return EV_INCOMPLETE;
  {
    const char* const v = "HTTP/1.";
    for (uint32_t i = 0; i < 7; i++)
      if (b[p + i] != (uint8_t)v[i]) return EV_ERROR;
    const uint32_t d = b[p + 7];
    if (d < '0' || d > '9') return EV_ERROR;
    rq.minor = d - '0';
    p += 8;
  }
  if (b[p] == '\r') {
    p++;
    if (p == E) return EV_INCOMPLETE;
    if (b[p++] != '\n') return EV_ERROR;
  } else if (b[p] == '\n') {
    p++;
  } else {
    return EV_ERROR;
  }
  for (uint32_t nh = 0;; nh++) {
    if (p == E) return EV_INCOMPLETE;
    uint32_t c = b[p];
    if (c == '\r') {
      p++;
      if (p == E) return EV_INCOMPLETE;
      if (b[p++] != '\n') return EV_ERROR;
      break;
    }
    if (c == '\n') {
      p++;
      break;
    }
    if (nh == MAX_HEADERS) return EV_ERROR;
    const bool named = !(nh != 0 && (c == ' ' || c == '\t'));
    uint32_t n0 = p, nl = 0;
    if (named) {
      for (;;) {
        c = b[p];
        if (c == ':') break;
        if (!is_token_char(c)) return EV_ERROR;
        p++;
        if (p == E) return EV_INCOMPLETE;
      }
      nl = p - n0;
      if (nl == 0) return EV_ERROR;
      p++;
      for (;;) {
        if (p == E) return EV_INCOMPLETE;
        c = b[p];
        if (!(c == ' ' || c == '\t')) break;
        p++;
      }
    }
    const uint32_t v0 = p;
    for (;;) {
      if (p == E) return EV_INCOMPLETE;
      c = b[p];
      if ((c < 0x20 && c != '\t') || c == 0x7f) break;
      p++;
    }
    uint32_t vl;
    if (c == '\r') {
      p++;
      if (p == E) return EV_INCOMPLETE;
      if (b[p++] != '\n') return EV_ERROR;
      vl = p - 2 - v0;
    } else if (c == '\n') {
      vl = p - v0;
      p++;
    } else {
      return EV_ERROR;
    }
    while (vl && (b[v0 + vl - 1] == ' ' || b[v0 + vl - 1] == '\t')) vl--;
    check_header(b, ref, k, named, n0, nl, v0, vl);
  }
  rq.consumed = p;
  rq.method_off = tok[0][0];
  rq.method_len = tok[0][1];
  rq.path_off = tok[1][0];
  rq.path_len = tok[1][1];
  return EV_PARSED;
}

XYWS_HD uint32_t put_text(uint8_t* out, uint32_t at, const char* s, uint32_t n) {
  for (uint32_t i = 0; i < n; i++) out[at + i] = (uint8_t)s[i];
  return at + n;
}

// The verdict for b[0, E) (full: len >= max_request) and the whole response in
// resp[0, RESP_MAX) (resp_len bytes of it; the caller copies what fits).
template <class R>
XYWS_HD verdict evaluate(const R& b, uint32_t E, bool full, uint32_t policy, uint8_t* resp) {
  const bool ref = (policy & XYWS_ACC_REFERENCE) != 0;
  verdict v = {0, 0, 0, 0, 0, 0, 0, NO_KEY};
  request rq = {0, 0, 0, 0, 0, 0};
  checks k;
  const int ev = walk(b, E, ref, rq, k);
  if (ev == EV_INCOMPLETE && !full) return v;
  uint32_t reason = XYWS_ACR_NONE;
  if (ev == EV_ERROR) {
    reason = XYWS_ACR_PARSE;
  } else if (ev == EV_INCOMPLETE) {
    reason = XYWS_ACR_TOO_LONG;
  } else {
    uint32_t fail = k.fail;
    if (!span_is(b, rq.method_off, rq.method_len, XYWS_LIT("GET"), false)) fail |= 1u << XYWS_ACR_METHOD;
    if (ref ? rq.minor != 1 : rq.minor < 1) fail |= 1u << XYWS_ACR_VERSION;
    if (!ref) {
      if (!k.host) fail |= 1u << XYWS_ACR_HOST;
      if (!k.upgrade) fail |= 1u << XYWS_ACR_UPGRADE;
      if (!k.connection) fail |= 1u << XYWS_ACR_CONNECTION;
      if (k.keys != 1) fail |= 1u << XYWS_ACR_KEY;
      if (k.versions != 1) fail |= 1u << XYWS_ACR_WS_VERSION;
    }
    for (uint32_t r = XYWS_ACR_METHOD; r <= XYWS_ACR_WS_VERSION && !reason; r++)
      if (fail & (1u << r)) reason = r;
  }
  if (reason) {
    v.status = XYWS_ACC_REJECTED;
    v.reason = reason;
    if (ev == EV_PARSED) v.consumed = rq.consumed;  // refused by a check: the request still ends there
    uint32_t n = put_text(resp, 0, "HTTP/1.1 400 Bad Request\r\n", 26);
    v.http_status = 400;
    if (!ref) {
      if (reason == XYWS_ACR_WS_VERSION) {
        v.http_status = 426;
        n = put_text(resp, 0, "HTTP/1.1 426 Upgrade Required\r\nSec-WebSocket-Version: 13\r\n", 58);
      }
      n = put_text(resp, n, "Connection: close\r\nContent-Length: 0\r\n\r\n", 40);
    }
    v.resp_len = n;
    return v;
  }
  v.status = XYWS_ACC_ACCEPTED;
  v.http_status = 101;
  v.consumed = rq.consumed;
  v.path_off = rq.path_off;
  v.path_len = rq.path_len;
  v.key_off = k.key_off;
  uint32_t kw[6];
  for (uint32_t i = 0; i < 6; i++) {
    uint32_t x = 0;
    for (uint32_t j = 0; j < 4; j++)
      x = (x << 8) | (k.key_off != NO_KEY ? b[k.key_off + 4 * i + j] : (uint8_t)"XXXXXXXXXXXXXXXXXXXXXX=="[4 * i + j]);
    kw[i] = x;
  }
  const uint32_t n = put_text(resp, 0,
                              "HTTP/1.1 101 Switching Protocols\r\nUpgrade: websocket\r\nConnection: Upgrade\r\n"
                              "Sec-WebSocket-Accept: ",
                              RESP_101_KEY);
  accept_value(kw, resp + n);
  v.resp_len = put_text(resp, n + 28, "\r\n\r\n", 4);
  return v;
}

XYWS_HD void to_result(const verdict& v, uint64_t out_cap, xyws_accept_result* r) {
  r->status = v.status | (v.resp_len > out_cap ? XYWS_ACC_TRUNCATED : 0u);
  r->http_status = (uint16_t)v.http_status;
  r->reason = (uint16_t)v.reason;
  r->consumed = v.consumed;
  r->resp_len = v.resp_len;
  r->path_off = v.path_off;
  r->path_len = v.path_len;
  r->key_off = v.key_off;
  r->reserved = 0;
}

// xyws_accept_request (include/xyws.h).
inline int accept_request(const void* host_req, uint64_t len, uint32_t max_request, uint32_t policy, void* host_out,
                          uint64_t out_cap, xyws_accept_result* res) {
  if (!args_ok(max_request, policy) || (len && !host_req) || (out_cap && !host_out)) return XYWS_ERR_INVALID;
  const uint32_t E = len < max_request ? (uint32_t)len : max_request;
  uint8_t resp[RESP_MAX];
  const verdict v = evaluate(host_bytes{(const uint8_t*)host_req}, E, len >= max_request, policy, resp);
  const uint64_t w = v.resp_len < out_cap ? v.resp_len : out_cap;
  for (uint64_t i = 0; i < w; i++) ((uint8_t*)host_out)[i] = resp[i];
  if (res) to_result(v, out_cap, res);
  return XYWS_OK;
}

}  // namespace xyws_accept
