/* shd_pcap.c -- the pcap files of captured hosts (include/shdtcp.h
 * shd_pcap_format / shd_pcap_write_host): utility/pcap_writer.c:19-137
 * restated byte for byte from the capture records the TCP path returns
 * (shd_tcp_result.pcap_records).
 *
 *   global header        pcap_writer.c:19-43 (fields in host byte order)
 *   record header        :50-70 (ts_sec, ts_usec, incl_len, orig_len)
 *   Ethernet, IP, TCP    :72-130 (fixed MACs; no checksums; 14 option bytes)
 *   file name            network_interface.c:641-647, pcap_writer.c:139-176
 *
 * The reference's fields are in network byte order where a real header's are
 * (its addresses and ports are in_addr_t / in_port_t, its lengths and
 * sequence numbers go through htons / htonl); the records here hold host
 * byte order, so every such field is converted on the way out.  Plain C: no
 * device code. */
#include <arpa/inet.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/shdtcp.h"

enum { kGlobalHdr = 24, kRecHdr = 16, kPktHdr = 66 };   /* 66: CONFIG_HEADER_SIZE_TCPIPETH */

static uint8_t* put(uint8_t* p, const void* v, size_t n) {
    memcpy(p, v, n);
    return p + n;
}

static uint8_t* put_global_header(uint8_t* p) {
    const uint32_t magic = 0xA1B2C3D4u, sigfigs = 0, snaplen = 65535, network = 1;
    const uint16_t major = 2, minor = 4;
    const int32_t zone = 0;
    p = put(p, &magic, 4);
    p = put(p, &major, 2);
    p = put(p, &minor, 2);
    p = put(p, &zone, 4);
    p = put(p, &sigfigs, 4);
    p = put(p, &snaplen, 4);
    return put(p, &network, 4);
}

size_t shd_pcap_format(const shd_pcap_rec* recs, uint64_t n, uint32_t flags, int32_t with_header, uint8_t* buf,
                       size_t cap) {
    const int headers_only = (flags & SHD_PCAP_HEADERS_ONLY) != 0;
    size_t need = with_header ? kGlobalHdr : 0;
    if (n && !recs) return 0;
    for (uint64_t i = 0; i < n; i++) need += kRecHdr + kPktHdr + (headers_only ? 0u : recs[i].len);
    if (!buf || cap < need) return need;
    uint8_t* p = buf;
    if (with_header) p = put_global_header(p);
    for (uint64_t i = 0; i < n; i++) {
        const shd_pcap_rec* r = &recs[i];
        const uint32_t ts_sec = (uint32_t)(r->time / 1000000000ull);
        const uint32_t ts_usec = (uint32_t)((r->time % 1000000000ull) / 1000ull);
        const uint32_t orig_len = kPktHdr + r->len;
        const uint32_t incl_len = headers_only ? (uint32_t)kPktHdr : orig_len;
        p = put(p, &ts_sec, 4);
        p = put(p, &ts_usec, 4);
        p = put(p, &incl_len, 4);
        p = put(p, &orig_len, 4);
        /* Ethernet */
        static const uint8_t mac[12] = {0x01, 0x23, 0x45, 0x67, 0x89, 0xAB, 0xA1, 0xB2, 0xC3, 0xD4, 0xE5, 0xF6};
        const uint16_t type = htons(0x0800);
        p = put(p, mac, 12);
        p = put(p, &type, 2);
        /* IP */
        const uint8_t ip0[2] = {0x45, 0x00}, ttl_proto[2] = {64, 6};
        const uint16_t total = htons((uint16_t)(orig_len - 14)), ident = 0, frag = 0x0040, sum = 0;
        const uint32_t sip = htonl(r->src_ip), dip = htonl(r->dst_ip);
        p = put(p, ip0, 2);
        p = put(p, &total, 2);
        p = put(p, &ident, 2);
        p = put(p, &frag, 2);
        p = put(p, ttl_proto, 2);
        p = put(p, &sum, 2);
        p = put(p, &sip, 4);
        p = put(p, &dip, 4);
        /* TCP */
        const uint16_t sport = htons(r->src_port), dport = htons(r->dst_port);
        const uint32_t seq = htonl(r->seq), ack = (r->flags & SHD_PCAP_ACK) ? htonl(r->ack) : 0;
        uint8_t off_flags[2] = {0x80, 0};
        if (r->flags & SHD_PCAP_RST) off_flags[1] |= 0x04;
        if (r->flags & SHD_PCAP_SYN) off_flags[1] |= 0x02;
        if (r->flags & SHD_PCAP_ACK) off_flags[1] |= 0x10;
        if (r->flags & SHD_PCAP_FIN) off_flags[1] |= 0x01;
        const uint16_t win = htons((uint16_t)r->win);
        p = put(p, &sport, 2);
        p = put(p, &dport, 2);
        p = put(p, &seq, 4);
        p = put(p, &ack, 4);
        p = put(p, off_flags, 2);
        p = put(p, &win, 2);
        memset(p, 0, 2 + 14);   /* checksum, options */
        p += 2 + 14;
        if (!headers_only && r->len) {   /* lengths are simulated, not content */
            memset(p, 0, r->len);
            p += r->len;
        }
    }
    return need;
}

/* <dir>/<hostname>-<a.b.c.d>.pcap (pcap_writer.c:139-165); NULL when out of memory */
static char* file_name(const char* dir, const char* hostname, uint32_t ip) {
    const char* d = dir ? dir : "data/pcapdata/";
    const size_t dl = strlen(d), n = dl + strlen(hostname) + 32;
    char* s = (char*)malloc(n);
    if (!s) return NULL;
    snprintf(s, n, "%s%s%s-%u.%u.%u.%u.pcap", d, (dl && d[dl - 1] == '/') ? "" : "/", hostname, (ip >> 24) & 255,
             (ip >> 16) & 255, (ip >> 8) & 255, ip & 255);
    return s;
}

static int write_file(const char* dir, const char* hostname, uint32_t ip, const shd_pcap_rec* recs, uint64_t n,
                      uint32_t flags) {
    const size_t need = shd_pcap_format(recs, n, flags, 1, NULL, 0);
    uint8_t* buf = (uint8_t*)malloc(need);
    char* name = file_name(dir, hostname, ip);
    int rc = 0;
    if (!buf || !name) {
        rc = -12;
    } else {
        shd_pcap_format(recs, n, flags, 1, buf, need);
        FILE* f = fopen(name, "w");
        if (!f) {
            fprintf(stderr, "shd_pcap_write_host: cannot open '%s' for writing\n", name);
            rc = -2;
        } else {
            if (fwrite(buf, 1, need, f) != need) rc = -5;
            if (fclose(f) != 0) rc = -5;
        }
    }
    free(name);
    free(buf);
    return rc;
}

int shd_pcap_write_host(const char* dir, const char* hostname, uint32_t ip, const shd_pcap_rec* recs, uint64_t n,
                        uint32_t flags) {
    if (!hostname || (n && !recs)) return -22;
    /* host.c:166-167 brings up the loopback interface first, then the ethernet one */
    const int rc = write_file(dir, hostname, 0x7F000001u, NULL, 0, flags);
    if (rc) return rc;
    return write_file(dir, hostname, ip, recs, n, flags);
}
