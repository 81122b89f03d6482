/*
 * shdtcp.h -- the TCP path on the GPU, C ABI.
 *
 * Runs the reference's TCP (host/descriptor/tcp.c, tcp_cong_reno.c,
 * tcp_retransmit_tally.cc, the socket buffers of socket.c and the interface of
 * network_interface.c) for client/server processes running the reference's own
 * TCP test application (src/test/tcp/test_tcp.c, nonblocking-epoll: connect,
 * send N bytes, read them echoed back, close) on every host of a model, in
 * conservative rounds on one GPU: one lane per host, a round is every event
 * before the window's end (the smallest path latency), deliveries cross hosts
 * through a mailbox between rounds.  Results equal the reference's serial loop
 * (tests/test_tcp_gpu.py against tests/golden/ref_tcp.json).  A bootstrap
 * period (<shadow bootstraptime>: no drops, no token buckets before its end)
 * and per-host heartbeat intervals (<host heartbeatfrequency>) run as the
 * reference's loop runs them (shd_tcp_model.bootstrap_end / host_heartbeat;
 * tests/test_tcp_options_gpu.py against tests/golden/ref_tcp_options.json).
 *
 * What a run says about its connections without tracing: with
 * SHD_TCP_OPT_FLOWS in shd_tcp_model.options, one flow record (shd_tcp_flow)
 * for every TCP connection endpoint -- when it opened, was established, last
 * delivered payload and sent its FIN, what it created, retransmitted and lost
 * and where -- written by the owning host's lane as the run goes and gathered
 * on the device at the end (shd_tcp_result_flows; tests/test_tcp_flows_gpu.py
 * against tests/golden/ref_tcp_flows.json).  A client's completion time is
 * t_last_delivered once bytes_delivered == tcp_bytes.  test_tcp.c closes
 * right after its last read, so t_fin equals it -- unless the socket still
 * held output at the close (the FIN follows once that has drained), or the
 * server's FIN overtook retransmitted data (the client's answer to it carries
 * FIN and comes before the last delivery): 6 of the fixture's 97 completed
 * clients.
 *
 * What a run says about its paths without tracing: with SHD_TCP_OPT_PATHS in
 * shd_tcp_model.options, one path record (shd_tcp_path) for every ordered pair
 * of vertices over which a host handed a packet to worker_sendPacket -- the
 * packets and bytes the network carried and the ones it lost, TCP packets and
 * the datagrams of a mixed model alike -- counted by the sending host's lane
 * where INET_SENT / INET_DROPPED are raised, summed per pair in a table on the
 * device and gathered at the end (shd_tcp_result_paths;
 * tests/test_tcp_paths_gpu.py against tests/golden/ref_tcp_paths.json).  With
 * path_cache the sends also go into the cache's packet counter
 * (shd_pc_packet_count: the reference's Path.packetCount).
 *
 * What a run says about where its packets waited without tracing: with
 * SHD_TCP_OPT_HOSTS in shd_tcp_model.options, one host record
 * (shd_tcp_hostrec) for every host -- what its upstream router queue (CoDel,
 * the one place the reference models congestion) took in, handed on and
 * dropped, how deep it got and how long the packets sat in it (sum, maximum
 * and a 16-bucket histogram of the sojourn), what the interface received,
 * dropped and sent, and how often a socket throttled a segment or took one
 * out of order -- counted by the host's own lane where the reference raises
 * the status, TCP packets and the datagrams of a mixed model alike, and copied
 * to the host at the end (shd_tcp_result_hosts; tests/test_tcp_hosts_gpu.py
 * against tests/golden/ref_tcp_hosts.json).  With SHD_TCP_OPT_HOST_SERIES
 * beside it, a sample of each host's record for every interval in which it
 * changed says when the queue built up (shd_host_sample,
 * shd_tcp_model.host_series_interval_us, shd_tcp_result_host_series;
 * tests/test_tcp_hseries_gpu.py against tests/golden/ref_tcp_hseries.json).
 *
 * A host's shape comes from the model.  Its socket slots are the sockets it
 * can ever create -- a socket is not released in a TCP run: for each of its
 * server processes the listener and one child per client process that names
 * it as its peer, one per client process of its own, and 16 for a datagram
 * process (its own socket and the per-datagram sockets waiting at the
 * interface); a host without processes has none.  The slots, the processes of
 * a host and its interface's queue of sockets wanting to send are ranges of
 * engine-wide arrays, so one hub host may serve dozens of clients beside
 * thousands of single-client hosts that hold one slot each
 * (shd_tcp_result.max_host_sockets / max_host_procs / sock_bytes;
 * tests/test_tcp_hub_gpu.py against tests/golden/ref_tcp_hub.json).  What
 * stays fixed is a listener's pending and child lists of 8: a server named
 * by more than eight clients whose connections are all open before it accepts
 * one ends the run with SHD_TCP_ERR_SOCKETS.
 *
 * The boundary is the same one shdgpu.h draws for the UDP path: plain
 * pointers and sizes, no torch types.  Path latency and reliability per host
 * pair come either from libshdgpu's path cache itself (path_cache set: the
 * lazy cache's first-touch rule applied on the device, round by round, as the
 * UDP engine does -- DESIGN.md §4), or from caller tables (Shadow's
 * topology_getLatency / topology_getReliability, topology.c:2053-2092, or
 * shd_pc_lookup), resolved in the order the serial loop touches them.
 */
#ifndef SHD_TCP_H
#define SHD_TCP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct shd_tcp_model {
    int32_t n_hosts, n_procs;
    const uint32_t* host_ip;          /* [H] host byte order (dns.c's addresses)        */
    const uint32_t* host_seed;        /* [H] host RNG state after attach                */
    const uint64_t* bw_down_kibps;    /* [H]                                            */
    const uint64_t* bw_up_kibps;      /* [H]                                            */
    int32_t n_vertices;               /* V: the attached vertices the tables index      */
    int32_t host_series_cap;          /* SHD_TCP_OPT_HOST_SERIES: records of the sample array
                                         (host_series_interval_us, below)                */
    const int32_t* host_vertex;       /* [H] each host's vertex index in [0, V)         */
    const double* path_lat_ms;        /* [V*V] src_vertex*V + dst_vertex; < 0: no route
                                         (pairs no host pair uses may be left < 0)       */
    const double* path_rel;           /* [V*V]                                          */
    const int32_t* proc_host;         /* [P] the host of each process, <process> order  */
    const uint64_t* proc_start;       /* [P] start time (ns)                            */
    const int32_t* proc_peer;         /* [P] -1: server; else the server process index  */
    uint64_t end_time;                /* ns; events at or past it are never run         */
    uint64_t heartbeat_interval;      /* ns (tracker heartbeats consume event IDs)      */
    uint32_t tcp_bytes;               /* bytes each client sends (test_tcp.c BUFFERSIZE) */
    uint32_t recv_buf, send_buf;      /* initial socket buffers (CONFIG_*_BUFFER_SIZE)   */
    uint32_t tcp_window;              /* --tcp-windows (options.c:79)                    */
    uint32_t packets_per_host;        /* packet pool per host (0: 8192); more live packets
                                         set SHD_TCP_ERR_POOL                             */
    uint32_t qdisc;                   /* --interface-qdisc (options.c:162): 0 fifo, 1 rr
                                         (network_interface.c:466-517)                    */
    uint32_t options;                 /* SHD_TCP_OPT_* bits; the others are reserved and ignored */
    /* SHD_TCP_OPT_HOST_SERIES: the sampling interval I of the host records'
     * series in microseconds (I = 1000 * host_series_interval_us ns; nonzero
     * with the option, ignored without), by the packet engine's rule
     * (shdgpu.h SHD_QF_HOST_SERIES).  The boundaries are T_k = k * I, k >= 1,
     * T_k < end_time; a model with end_time / I >= 2^32 is refused (-22).  A
     * host's record is touched by each of the eight statuses it counts
     * (shd_tcp_hostrec).  A touch at t yields one shd_host_sample labelled
     * with the first boundary after it, (t / I + 1) * I -- a status raised at
     * exactly T_k belongs to the interval after it -- holding the host's whole
     * record after every one of its events before that boundary, depth_end
     * the queue's length then.  An interval without a touch yields no sample,
     * and neither does a boundary that is not before end_time.  The host's
     * own lane appends the samples to one engine-wide array in device memory,
     * emptied into host memory where the flow series' array is (shd_tcp_run:
     * after every batch of 64 rounds; a group: after 64 rounds at the latest,
     * or once the array is past half), so a series is as long as the run.
     * host_series_cap: records of that array, 240 bytes each (<= 0: the
     * default, the larger of 2^18 and sixteen per host of the engine; at most
     * 2^24, more is refused with -22).  Sizing rule: between two drains a
     * host appends at most one sample per boundary it crosses with a touch:
     * a round's touches lie within one window W (the smallest path latency),
     * so no more than 64 * (W / I + 1) per host of the engine, and seldom
     * more than one at an interval above W.  An append that finds the array
     * full writes nothing and sets
     * SHD_TCP_ERR_HSERIES.  (The field sits in what was padding after
     * `options`, and host_series_cap in the padding after n_vertices: the
     * struct keeps its size and every other field its offset, so a caller
     * built against the older header passes the same bytes; both are read
     * only with the option's bit.  Such a caller's uninitialised padding is
     * harmless only because bit 16 of `options` was reserved and ignored: a
     * caller that set that bit by accident is now refused with -22 or runs
     * with the series.) */
    uint32_t host_series_interval_us;
    /* A built path cache of this model's graph (shdgpu.h shd_pc_create: an
     * undirected graph, the hosts' vertices attached), or NULL.  Set: every
     * path query of the run goes to the cache's device tables under the lazy
     * cache's first-touch rule (topology.c:1969-2051): a pair with a ranked
     * endpoint at the round's start takes the lower-ranked endpoint's row; a
     * pair with none takes the querying source's row, the query logged with
     * its event key, and between rounds the log is ranked in serial order
     * (event_compare's key, then the query's index within its event), which
     * both checks every such choice and ranks the rows that ran.  A choice the
     * serial order contradicts (two unranked endpoints first touched from both
     * sides within one window) ends the run with SHD_TCP_ERR_FIRST_TOUCH; the
     * caller then runs the model on tables (the fields above).  The cache's
     * ranks are left as the serial run leaves them.  host_vertex then holds
     * graph vertex ids, and n_vertices / path_lat_ms / path_rel are unused. */
    struct shd_pc* path_cache;
    /* Datagram processes beside the echo ones: both transports in one model,
     * on each host's one interface (qdisc, token buckets, CoDel queue) --
     * network_interface.c:519-579 serves TCP and UDP sockets alike.
     * proc_app[k] >= 0: process k runs the datagram application
     * app_spec[4 * proc_app[k] ..] = shd_udp_app's {send, dest, n_start,
     * per_read} (shdgpu.h; PHOLD's port 8998) instead of the echo, with
     * proc_peer[k] = -1; at most one such process per host.  NULL proc_app:
     * every process runs the echo.  udp_payload: bytes per datagram (1 ..
     * 65507); app_peer [H]: the SHD_DEST_PEER host of each host; dest_cum
     * [n_classes][H] / host_class [H]: SHD_DEST_WEIGHTED's cumulative weights
     * (host_class NULL: row 0).  A datagram process adds 16 socket slots to
     * its host (the file comment's rule): more per-datagram sockets waiting
     * at the interface at once set SHD_TCP_ERR_SOCKETS. */
    const int32_t* proc_app;
    const uint32_t* app_spec;
    int32_t n_app_specs;
    uint32_t udp_payload;
    const int32_t* app_peer;
    const double* dest_cum;
    const uint8_t* host_class;
    int32_t n_classes;
    /* SHD_TCP_OPT_SERIES: records of the engine's sample array (<= 0: the
     * default, the larger of 2^20 and four per socket slot of the engine's
     * hosts; at most 2^26, more is refused with -22).  96 bytes each.  It must
     * hold what the hosts append between two drains (series_interval_us). */
    int32_t series_cap;
    /* Packet capture (the reference's <host logpcap="true">,
     * network_interface.c:337-373): pcap_host[h] != 0 makes host h a capture
     * host; NULL: none.  A capture host's lane writes one shd_pcap_rec for
     * every packet its interface sends (after the packet went to the router
     * or the loopback task, :571-574) and receives (after its socket processed
     * it, :415-418; the loopback delivery too) into that host's ring of
     * pcap_ring records in device memory (0: 65 536); the rings exist for the
     * capture hosts only, and a model with none allocates nothing and runs
     * the rounds as before.  The rings are emptied into host memory between
     * batches of rounds (shd_tcp_run: after every batch of 64; a group: after
     * 64 rounds at the latest, or once a ring is past half), so a capture is
     * as long as the run; a ring that fills between two drains sets
     * SHD_TCP_ERR_PCAP.  Capture works with and without trace.  The
     * reference's capture reads every packet's TCP header and asserts on a
     * datagram (network_interface.c:348, packet.c:485-489): a model with a
     * capture host and a datagram process is refused (-22). */
    const uint8_t* pcap_host;
    uint32_t pcap_ring;
    /* SHD_TCP_OPT_SERIES: the sampling interval I in microseconds (I = 1000 *
     * series_interval_us ns; nonzero with the option, ignored without).  The
     * boundaries are T_k = k * I, k >= 1, T_k < end_time.  A flow record is
     * touched when one of the six statuses its counters count is attributed to
     * it (shd_tcp_flow: SND_CREATED, SND_TCP_RETRANSMITTED, INET_DROPPED,
     * RCV_SOCKET_DELIVERED, RCV_SOCKET_DROPPED, ROUTER_DROPPED; setting
     * t_established does not count).  A touched record yields one
     * shd_tcp_sample labelled with the first boundary after the touch -- an
     * event at exactly T_k belongs to the interval after it -- holding the
     * record's cumulative counters after every event of its host before that
     * boundary.  An interval without a touch yields no sample: the series is
     * sparse and its reader fills forward.  A last touch whose boundary is not
     * before end_time yields none either: the flow record is the end state.
     * The owning host's lane appends the samples to one engine-wide array in
     * device memory (series_cap), which is emptied into host memory where the
     * capture rings are (shd_tcp_run: after every batch of 64 rounds; a group:
     * after 64 rounds at the latest, or once the array is past half), so a
     * series is as long as the run; an append that finds the array full sets
     * SHD_TCP_ERR_SERIES and writes nothing. */
    uint32_t series_interval_us;
    /* The bootstrap period (<shadow bootstraptime>, shd_model.bootstrap_end):
     * ns, 0 for none.  worker_isBootstrapActive() is now < bootstrap_end
     * (worker.c:462-466: strict, at the executing event's time), read once
     * where each of these begins:
     *   worker_sendPacket (worker.c:281-290): the reliability is queried and
     *     the random draw taken as always (first touches and the RNG stream do
     *     not change); the packet passes if bootstrapping || chance <=
     *     reliability || payload == 0;
     *   _networkinterface_receivePackets (network_interface.c:431-454): the
     *     loop is while (bootstrapping || receive bucket >= MTU); while
     *     bootstrapping the bucket is not consumed and no refill is scheduled
     *     (the router queue still dequeues through CoDel);
     *   _networkinterface_sendPackets (network_interface.c:522-569): the
     *     loop's condition stays send bucket >= MTU, with no "bootstrapping ||";
     *     only the consume and the refill scheduling are skipped, for the
     *     loopback +1 ns task's packets too.  Tracker counters and capture run
     *     as always.
     * Refill events stop by themselves once the buckets are full and start
     * again with the first consume after the period, which the hosts' event-ID
     * counters show.  The same value on every rank of a group. */
    uint64_t bootstrap_end;
    /* [H] each host's own heartbeat interval in ns (<host heartbeatfrequency>,
     * host.c's heartbeatInterval; shd_model.host_heartbeat), or NULL:
     * heartbeat_interval for every host.  The tracker's boot line and each
     * heartbeat (tracker.c:141, 566-611) then come at the host's own interval;
     * the [node] line's first field is that interval in whole seconds (a
     * 500 ms host prints 0).  A zero entry is refused (-22), as
     * shd_eng_create refuses one.  node_k is sized from the smallest interval
     * among the engine's hosts; a group's rank reads its hosts' slice. */
    const uint64_t* host_heartbeat;
} shd_tcp_model;

/* one captured packet: what _networkinterface_capturePacket takes from the
 * packet's TCP header (addresses and ports in host byte order here), the time
 * it was captured and the direction; shd_pcap_format makes the file's bytes */
typedef struct shd_pcap_rec {
    uint64_t time;                    /* ns */
    uint32_t src_ip, dst_ip;
    uint32_t seq, ack, win;           /* as the packet holds them (ack also when ACK is clear) */
    uint16_t src_port, dst_port;
    uint16_t len;                     /* payload bytes */
    uint8_t flags;                    /* SHD_PCAP_RST | _SYN | _ACK | _FIN */
    uint8_t dir;                      /* SHD_PCAP_IN / SHD_PCAP_OUT */
    uint32_t _pad;
} shd_pcap_rec;
enum { SHD_PCAP_RST = 1, SHD_PCAP_SYN = 2, SHD_PCAP_ACK = 4, SHD_PCAP_FIN = 8 };
enum { SHD_PCAP_IN = 0, SHD_PCAP_OUT = 1 };

/* the first path query a host made of a vertex pair (topology_isRoutable /
 * getLatency / getReliability): the executing event's key (event_compare:
 * time, host, src, seq) and the query's index within that event; the caller
 * ranks the run's first touches in this order (shadow-1_amd/tcp.py) */
typedef struct shd_tcp_query {
    uint64_t time, seq;
    uint32_t host, src, index;
    int32_t v_src, v_dst;             /* vertex indices (path table) of the query       */
    uint32_t _pad;
} shd_tcp_query;

typedef struct shd_tcp_result {
    char* lines;                      /* "<time>\t<host>\t[STATUS] ...\n", each host's lines in
                                         its execution order, hosts in index order           */
    size_t len;
    uint64_t n_lines;
    uint64_t* next_event_id;          /* [H] host event counter at the end                */
    uint64_t* next_packet_id;         /* [H]                                              */
    uint32_t* rng_probe;              /* [H] the next rand_r value of each host RNG       */
    uint64_t rounds;                  /* conservative rounds run                          */
    uint64_t events;                  /* events executed                                  */
    double device_ms;                 /* GPU time of the rounds (HIP events)              */
    uint32_t error;                   /* SHD_TCP_ERR_* bits; nonzero: results invalid     */
    uint64_t deliveries;              /* packets handed to a receiving host (worker.c:260-321's
                                         delivery events executed)                           */
    shd_tcp_query* queries;           /* each host's first query of each vertex pair      */
    uint64_t n_queries;
    /* with SHD_TCP_TRACE_NODE: the tracker's node counters of every heartbeat
     * interval (tracker.c:183-214, 566-611), [H][node_k][20]: inbound remote
     * then outbound remote, each packets-control, bytes-control-header,
     * packets-control-retrans, bytes-control-header-retrans, packets-data,
     * bytes-data-header, bytes-data-payload, packets-data-retrans,
     * bytes-data-header-retrans, bytes-data-payload-retrans; a host's packets
     * to its own address (the loopback task, network_interface.c:548-555) are
     * counted here as the reference counts them: remote, since tracker.c:223
     * and :255 call a packet local only when its address is 127.0.0.1, which
     * no model's sockets use, so the localhost counters are zero.
     * n_heartbeats[h] of them are host h's, one per interval of that host's
     * own (shd_tcp_model.host_heartbeat).
     * shd_tracker_node_lines (shdgpu.h) makes the [node] lines of a host from
     * them and the host's interval. */
    uint64_t* node_counters;
    uint32_t* n_heartbeats;
    uint32_t node_k;
    uint32_t first_touch_reruns;      /* path_cache mode: runs this call made again from the start,
                                         each with one more round's first touches ranked in
                                         serial order before it runs (a contradicted device
                                         choice that changed a value) */
    uint64_t max_round_deliveries;    /* the most deliveries one round's mailbox took */
    uint64_t max_round_overflow;      /* ... and the most of them in its shared overflow range */
    double setup_ms, results_ms, teardown_ms;   /* the call's host wall time around the rounds:
                                                   allocation and upload, copies back and
                                                   formatting, release */
    /* the hosts this result covers: [first_host, first_host + n_local_hosts)
     * (shd_tcp_run: all of them; shd_tcp_run_group: this engine's share) --
     * the per-host arrays above (next_event_id, next_packet_id, rng_probe,
     * node_counters, n_heartbeats) and the lines are these hosts'; the lines
     * carry the model's host index.  queries: every engine's. */
    int32_t first_host, n_local_hosts;
    /* the capture records of this result's hosts (shd_tcp_model.pcap_host):
     * hosts in index order, each host's records in its interface's order;
     * host first_host + i's are pcap_records[pcap_off[i] .. pcap_off[i + 1]).
     * NULL / NULL when the model has no capture host.  pcap_drains: the times
     * the rings were emptied with something in them; pcap_ring_peak: the most
     * records one host's ring held at a drain. */
    shd_pcap_rec* pcap_records;
    uint64_t* pcap_off;               /* [n_local_hosts + 1] */
    uint64_t pcap_drains;
    uint32_t pcap_ring_peak, _pad11;
    /* the shape the model gave this result's hosts (the file comment's rule):
     * the most socket slots one of them used and the most processes one of
     * them runs; sock_bytes: device bytes of this engine's socket slots,
     * SHD_TCP_SOCK_BYTES for each slot of the rule's sum over its hosts */
    uint32_t max_host_sockets;
    uint32_t max_host_procs;
    uint64_t sock_bytes;
} shd_tcp_result;

/* One TCP connection endpoint of a run with SHD_TCP_OPT_FLOWS: every TCP
 * socket that ever created a packet -- a connecting socket, and a listener's
 * child from its SYN+ACK on; listeners and datagram sockets have none.  Times
 * are ns, 0: never.  Every field but the last five is counted where the
 * reference raises a packet status (packet_addDeliveryStatus) or sets the
 * state, so it can be read off a traced run's [STATUS] lines
 * (tests/tcp_flow_expect.py):
 *   t_open            the socket's first SND_CREATED (tcp.c:791-835)
 *   t_established     its _tcp_setState(ESTABLISHED) (tcp.c:1865, 1887)
 *   t_last_delivered, bytes_delivered
 *                     RCV_SOCKET_DELIVERED (tcp.c:2226, 2266): the last one's
 *                     time, the payload of all of them
 *   t_fin             the first SND_CREATED of a packet carrying FIN
 *   packets_created, bytes_created
 *                     SND_CREATED: count and payload (a retransmission sends
 *                     the same packet again and is not counted again)
 *   retransmitted     SND_TCP_RETRANSMITTED (tcp.c:1060)
 *   inet_dropped      INET_DROPPED of its packets (worker.c:281-290)
 *   socket_dropped    RCV_SOCKET_DROPPED of packets addressed to it
 *   router_dropped    ROUTER_DROPPED, at this host, of packets addressed to
 *                     this endpoint's 4-tuple.  The lane finds the record by
 *                     the 4-tuple among its host's records (what the
 *                     interface's lookup and a listener's child list give while
 *                     the socket lives, and a closed child still: the
 *                     reference raises the status for such a packet too); a
 *                     packet addressed to no record is counted nowhere
 * role: 0 its first packet is a SYN without ACK (a connecting socket), 1 a
 * listener's child.  proc: the connecting process, or for a child the server
 * process that listens.  local_* / peer_*: the addresses its packets carry
 * (host byte order).
 * state, cwnd, ssthresh, srtt, rttvar are the socket's values when the run
 * ends (state: 0 CLOSED, 1 LISTEN, 2 SYNSENT, 3 SYNRECEIVED, 4 ESTABLISHED,
 * 5 FINWAIT1, 6 FINWAIT2, 7 CLOSING, 8 TIMEWAIT, 9 CLOSEWAIT, 10 LASTACK, the
 * order of tcp.c's enum TCPState; cwnd and ssthresh in segments; srtt and
 * rttvar in ms).  They are
 * what the reference's tcp_getInfo exports as tcpi_state, tcpi_snd_cwnd,
 * tcpi_snd_ssthresh, tcpi_rtt and tcpi_rttvar (tcp.c:1409-1459).  The pin has
 * two links: the oracle's values equal the reference's wherever a process can
 * observe its socket -- each time it runs, from the socket's creation until
 * the process closes it (tests/test_tcp_snapshots_ref_cpu.py) -- and the
 * records equal the oracle's change log at the end of the run
 * (tests/test_tcp_snapshots_gpu.py).  What follows the close (the FIN
 * exchange, TIMEWAIT, CLOSED) no reference process observes: it is pinned
 * oracle-to-device only. */
typedef struct shd_tcp_flow {
    int32_t host, proc;               /* the model's host index; process index      */
    uint32_t local_ip, peer_ip;
    uint16_t local_port, peer_port;
    uint8_t role, state;
    uint16_t _pad;
    uint64_t t_open, t_established, t_last_delivered, t_fin;
    uint64_t bytes_delivered, packets_created, bytes_created;
    uint64_t retransmitted, inet_dropped, socket_dropped, router_dropped;
    uint32_t cwnd, ssthresh;
    int32_t srtt, rttvar;
} shd_tcp_flow;

/* One sample of a run with SHD_TCP_OPT_SERIES (shd_tcp_model.
 * series_interval_us states the rule): flow record `flow` of the same result
 * (shd_tcp_result_flows' index) as it stood at boundary t -- the seven
 * counters of shd_tcp_flow, pinned by a traced run's [STATUS] lines
 * (tests/tcp_series_expect.py), and the socket's state, cwnd, ssthresh, srtt
 * and rttvar when the sample was taken (before the host's first event at or
 * past t, or at the end of the run): the oracle's change log just before t,
 * pinned as shd_tcp_flow's five are (tests/test_tcp_snapshots_gpu.py). */
typedef struct shd_tcp_sample {
    uint64_t t;                 /* the boundary T_k, ns */
    uint32_t flow;              /* index into shd_tcp_result_flows' array of the same result */
    int32_t  host;
    uint64_t bytes_delivered, packets_created, bytes_created;
    uint64_t retransmitted, inet_dropped, socket_dropped, router_dropped;
    uint32_t cwnd, ssthresh; int32_t srtt, rttvar;   /* the socket's values when the sample was taken */
    uint8_t  state, _pad[7];
} shd_tcp_sample;

/* what the drains of a run's sample array saw: the times it was emptied with
 * something in it, the most records one drain found, and its capacity */
typedef struct shd_tcp_series_info {
    uint64_t drains;
    uint32_t peak, capacity;
} shd_tcp_series_info;

/* One ordered vertex pair of a run with SHD_TCP_OPT_PATHS: what the hosts on
 * v_src handed to worker_sendPacket for hosts on v_dst (worker.c:260-321),
 * counted where the reference raises the packet's status, so every counted
 * packet is one INET_SENT or INET_DROPPED [STATUS] line of a traced run
 * (tests/tcp_path_expect.py).  A host's packets to its own address go through
 * the loopback task (network_interface.c:548-555), never reach
 * worker_sendPacket and are not counted; two hosts on one vertex give the
 * pair (v, v).  Datagrams of shd_udp_app processes count like TCP packets. */
typedef struct shd_tcp_path {
    int32_t v_src, v_dst;          /* shd_tcp_model.host_vertex of the sending and of the destination host */
    uint64_t packets_sent;         /* INET_SENT   (worker.c:290-306; counted where the status is raised,
                                      also when the delivery would fall past end_time) */
    uint64_t bytes_sent;           /* their payload (the line's bytes=) */
    uint64_t control_sent;         /* those of them with payload 0 (never dropped, worker.c:288-290) */
    uint64_t packets_dropped;      /* INET_DROPPED (worker.c:319) */
    uint64_t bytes_dropped;
    uint64_t t_first, t_last;      /* ns: first and last time worker_sendPacket handled a packet of the
                                      pair, either outcome; a record exists only for a pair that saw one */
} shd_tcp_path;

/* One host of a run with SHD_TCP_OPT_HOSTS: what its upstream router queue,
 * its interface and its sockets' two TCP queues did, each field counted by
 * the host's own lane where the reference raises the named status on that
 * host, so every count is a number of [STATUS] lines of a traced run that the
 * host executed (tests/tcp_host_expect.py).  Bytes are the packet's payload
 * (the line's bytes=).  TCP packets and the datagrams of a mixed model count
 * alike: the router and the interface serve both.  The router queue is FIFO
 * and never refuses a packet (CODEL_PARAM_QUEUE_SIZE_LIMIT is G_MAXUINT), so
 * every drop is a CoDel drop of the queue's head.  A host that saw no packet
 * has a record that is zero apart from `host`.  Times are ns. */
typedef struct shd_tcp_hostrec {
    int32_t  host;                  /* the model's host index */
    uint32_t depth_max;             /* the most packets the queue held right after a ROUTER_ENQUEUED, that packet included */
    uint32_t depth_end;             /* packets still queued when the run ended: enqueued - dequeued - dropped */
    uint32_t _pad;
    uint64_t router_enqueued, router_enqueued_bytes;   /* ROUTER_ENQUEUED (router.c:113) */
    uint64_t router_dequeued, router_dequeued_bytes;   /* ROUTER_DEQUEUED (router.c:129) */
    uint64_t router_dropped, router_dropped_bytes;     /* ROUTER_DROPPED (router_queue_codel.c:139) */
    uint64_t t_depth_max;           /* the first enqueue that reached depth_max */
    /* over the dequeued packets only: a packet's sojourn is its ROUTER_DEQUEUED
     * time minus its ROUTER_ENQUEUED time; t_sojourn_max is the first dequeue
     * that reached the maximum */
    uint64_t sojourn_sum, sojourn_max, t_sojourn_max;
    uint64_t if_received, if_received_bytes;   /* RCV_INTERFACE_RECEIVED (network_interface.c:382), the
                                                  loopback task's delivery included */
    uint64_t if_dropped;                       /* RCV_INTERFACE_DROPPED (:411) */
    uint64_t if_sent, if_sent_bytes;           /* SND_INTERFACE_SENT (:545), packets to the host's own address included */
    uint64_t tcp_throttled;         /* SND_TCP_ENQUEUE_THROTTLED (tcp.c:743) */
    uint64_t tcp_unordered;         /* RCV_TCP_ENQUEUE_UNORDERED (tcp.c:758) */
    uint64_t t_first, t_last;       /* first and last time one of the statuses above was raised on the host; 0: never */
    /* the dequeued packets by sojourn: bucket min(15, bit_length(sojourn >> 16)),
     * bit_length(0) = 0 -- bucket 0 below 65.536 us, bucket k [2^(15+k), 2^(16+k))
     * ns, bucket 15 2^30 ns (1.07 s) and above; they sum to router_dequeued */
    uint32_t sojourn_hist[16];
} shd_tcp_hostrec;

/* One sample of a host-record series (the packet engine's SHD_QF_HOST_SERIES,
 * shdgpu.h shd_eng_host_series, and the TCP path's SHD_TCP_OPT_HOST_SERIES,
 * shd_tcp_result_host_series): `rec` is host rec.host's whole record as it
 * stood after every event of the host before the boundary `t` (ns, a multiple
 * of the interval), depth_end the queue's length at `t`.  A host has a sample
 * for boundary t only if one of the record's statuses was raised on it in the
 * interval that ends at t (an event at exactly t belongs to the next one), so
 * a reader fills forward: the record at an unsampled boundary is the host's
 * last sample before it, and zero before its first. */
typedef struct shd_host_sample {
    uint64_t t;
    shd_tcp_hostrec rec;
} shd_host_sample;   /* 240 B */

/* shd_tcp_model.options: independent bits, but SHD_TCP_OPT_SERIES is valid only
 * together with SHD_TCP_OPT_FLOWS and a nonzero series_interval_us, and
 * SHD_TCP_OPT_HOST_SERIES only together with SHD_TCP_OPT_HOSTS and a nonzero
 * host_series_interval_us (-22 otherwise, before any device call) */
enum { SHD_TCP_OPT_FLOWS = 1, SHD_TCP_OPT_PATHS = 2, SHD_TCP_OPT_SERIES = 4, SHD_TCP_OPT_HOSTS = 8,
       SHD_TCP_OPT_HOST_SERIES = 16 };

/* The most entries the device's pair table gets (SHD_TCP_OPT_PATHS; 64 bytes
 * each: 256 MiB).  Its capacity is a power of two at least twice min(Vu^2, E +
 * 2 Vd Vu) -- Vu the distinct host_vertex values, E the distinct ordered
 * vertex pairs of the echo connections in both directions (a connection
 * within one host has none), Vd the distinct vertices of hosts with a
 * datagram process -- and at most this; SHD_TCP_PATH_SLOTS in the environment
 * forces it (tests).  A model with more pairs in use than entries ends with
 * SHD_TCP_ERR_PATHS.  SHD_TCP_PATH_TIMING in the environment (any value) makes
 * a run with the option print, on stderr, the number of records, the table's
 * capacity and the device time of the fold and the gather at its end
 * (measurements: profiles/paths/ab.txt). */
#define SHD_TCP_PATH_SLOTS_MAX (1u << 22)

/* device bytes of one socket slot (its buffers, queues, SACK and retransmit
 * state at their fixed capacities) */
#define SHD_TCP_SOCK_BYTES 141888

/* shd_tcp_run's `trace` bits */
enum { SHD_TCP_TRACE_STATUS = 1, SHD_TCP_TRACE_NODE = 2 };

enum {
    SHD_TCP_ERR_EVQ = 1, SHD_TCP_ERR_POOL = 2, SHD_TCP_ERR_QUEUE = 4,
    SHD_TCP_ERR_SOCKETS = 8,   /* a host created more sockets than its slots (a datagram process with more
                                  than 16 sockets at once), or a listener held more than 8 children */
    SHD_TCP_ERR_MAILBOX = 16, SHD_TCP_ERR_TRACE = 32, SHD_TCP_ERR_SACK = 64, SHD_TCP_ERR_INTERNAL = 128,
    SHD_TCP_ERR_QLOG = 256, SHD_TCP_ERR_FIRST_TOUCH = 512,
    SHD_TCP_ERR_PCAP = 1024,  /* a capture ring filled between two drains (pcap_ring) */
    SHD_TCP_ERR_PATHS = 2048, /* the device's pair table had no free entry for a vertex pair (SHD_TCP_OPT_PATHS):
                                 counts could not be placed, the path records are incomplete */
    SHD_TCP_ERR_SERIES = 4096, /* the sample array filled between two drains (SHD_TCP_OPT_SERIES, series_cap):
                                 the sample was not written, the series is incomplete */
    SHD_TCP_ERR_HSERIES = 8192 /* the host records' sample array filled between two drains
                                  (SHD_TCP_OPT_HOST_SERIES, host_series_cap): the sample was not written, and
                                  the series holds the samples appended before it only */
};

/* Run the model to end_time on the current HIP device (the reference's
 * src/main/core/worker.c loop for these processes; see the file comment).  trace & 1 writes the
 * [STATUS] lines (packet.c:647-659); trace & 2 keeps the tracker's node
 * counters per heartbeat (the [node] lines, tracker.c:419-465).  Returns 0 or a negative errno-style code:
 * -22 an invalid model, -113 a client whose server has no route in either
 * direction (the reference's connect fails with ECONNREFUSED there,
 * host.c:1224-1234; the device application has no such branch), -12 no device
 * memory for the trace buffers or the capture rings, -5 a HIP error.  A client on another host than
 * its server that starts less than one window W (the smallest path latency)
 * after it is refused (-22): it could connect in the round its server binds,
 * and the port it reads would depend on the lanes' timing.  *out is allocated by the call
 * and released by shd_tcp_result_free. */
int shd_tcp_run(const shd_tcp_model* m, int32_t trace, shd_tcp_result** out);
void shd_tcp_result_free(shd_tcp_result* r);

/* The flow records of the hosts this result covers (a result of shd_tcp_run /
 * shd_tcp_run_group only): by host index, then by the socket's slot within its
 * host (creation order), so a group's ranks concatenated in rank order equal
 * the one-engine array; a connection across ranks has one record on each
 * side.  *recs NULL and *n 0 when the model did not set SHD_TCP_OPT_FLOWS.
 * Owned by the result.  Returns 0, -22 for a NULL argument.  Without the
 * option a run allocates nothing for them, launches nothing extra and runs the
 * rounds as before; a rerun from the start (first_touch_reruns) starts the
 * records again with it. */
int shd_tcp_result_flows(const shd_tcp_result* r, const shd_tcp_flow** recs, uint64_t* n);

/* The path records of the hosts this result covers (a result of shd_tcp_run /
 * shd_tcp_run_group only): one for every ordered pair (v_src, v_dst) over
 * which one of them handed a packet to worker_sendPacket, sorted by (v_src,
 * v_dst).  A group's rank returns its own hosts' sends -- nothing is
 * exchanged -- so the ranks' records summed per pair (t_first min, t_last
 * max) are the one-engine records.  *recs NULL and *n 0 when the model did
 * not set SHD_TCP_OPT_PATHS.  Owned by the result.  Returns 0, -22 for a NULL
 * argument.  Without the option a run allocates nothing for them, launches
 * nothing extra and runs the rounds as before; a rerun from the start
 * (first_touch_reruns) starts the records again.
 * With path_cache and the option, a run that ends without an error bit adds
 * each pair's packets_sent to the cache's packet counter, keyed on the
 * unordered attached pair as shd_pc_count_packet keys it: afterwards
 * shd_pc_packet_count(pc, a, b) has grown by sent[a->b] + sent[b->a] (by
 * sent[a->a] once for a pair on one vertex), the reference's
 * Path.packetCount.  Once, after the last rerun; a group's rank adds its own
 * hosts' sends to its own cache, as shd_eng_path_counts documents for engine
 * groups. */
int shd_tcp_result_paths(const shd_tcp_result* r, const shd_tcp_path** recs, uint64_t* n);

/* The samples of the hosts this result covers (a result of shd_tcp_run /
 * shd_tcp_run_group only), sorted by (flow, t): `flow` indexes the array
 * shd_tcp_result_flows gives for the same result, so a group's rank returns
 * its own hosts' samples against its own flow array (the ranks concatenated
 * in rank order, each rank's `flow` offset by the records before it, are the
 * one-engine array).  info, when not NULL, takes the drains' figures.  *recs
 * NULL and *n 0 (info zero) when the model did not set SHD_TCP_OPT_SERIES.
 * Owned by the result.  Returns 0, -22 for a NULL r, recs or n.  Without the
 * option a run allocates nothing for the series, launches nothing extra and
 * the round's event loop tests one launch-uniform word; a rerun from the
 * start (first_touch_reruns) starts the series again with the records. */
int shd_tcp_result_series(const shd_tcp_result* r, const shd_tcp_sample** recs, uint64_t* n,
                          shd_tcp_series_info* info);

/* The host records of the hosts this result covers (a result of shd_tcp_run /
 * shd_tcp_run_group only): a dense array, *n == n_local_hosts, record i
 * describing host first_host + i, so a group's ranks concatenated in rank
 * order are the one-engine array -- nothing is exchanged between ranks.
 * *recs NULL and *n 0 when the model did not set SHD_TCP_OPT_HOSTS.  Owned by
 * the result.  Returns 0, -22 for a NULL argument.  The records have a fixed
 * size, so nothing can overflow and the option has no error bit.  Without the
 * option a run allocates nothing for them, launches nothing extra and runs
 * the rounds as before; a rerun from the start (first_touch_reruns) starts the
 * records again.  SHD_TCP_HOST_TIMING in the environment (any value) makes a
 * run with the option print, on stderr, the size and the host wall time of
 * the records' copy at its end (measurements: profiles/hosts/ab.txt). */
int shd_tcp_result_hosts(const shd_tcp_result* r, const shd_tcp_hostrec** recs, uint64_t* n);

/* The host records' series of the hosts this result covers (a result of
 * shd_tcp_run / shd_tcp_run_group only), sorted by (rec.host, t), rec.host the
 * model's host index and rec._pad 0: a group's rank returns its own hosts'
 * samples -- nothing is exchanged -- and the ranks' arrays joined and sorted
 * are the one-engine array.  A host whose last touched interval ends before
 * end_time has its final record as that boundary's sample.  info, when not
 * NULL, takes the drains' figures.  *recs NULL and *n 0 (info zero) when the
 * model did not set SHD_TCP_OPT_HOST_SERIES.  Owned by the result.  Returns 0,
 * -22 for a NULL r, recs or n.  Without the option a run allocates nothing
 * for the series and launches nothing extra; a rerun from the start
 * (first_touch_reruns) starts the series again with the records.
 * SHD_TCP_SERIES_TIMING in the environment (any value) makes a run with the
 * option print, on stderr, the samples, the drains and their host wall time. */
int shd_tcp_result_host_series(const shd_tcp_result* r, const shd_host_sample** recs, uint64_t* n,
                               shd_tcp_series_info* info);

/* The same model on a group of engines, one per process and GPU (shdgpu.h
 * shd_comm: RCCL, or the host-memory transport for several processes on one
 * GPU), every rank calling with the same model: rank r runs hosts
 * [r * H / world, (r + 1) * H / world) -- the reference's rounds across
 * workers (slave.c:437-462) with its hosts' events, both transports, the
 * qdisc, buckets and CoDel queue on the engine that owns the host.  Each
 * round's window starts at the earliest pending event over the group (an
 * all-gather of a few words per engine); after the round the deliveries for
 * other engines' hosts go to them: every engine writes them into one segment
 * per destination engine (SHD_TCP_XCAP deliveries per engine pair and round,
 * max(16384, 8 x the engine's hosts) by default; more set
 * SHD_TCP_ERR_MAILBOX), the segments' counts go round in one all-gather and
 * only their used parts in an all-to-all-v (grouped send / receive on RCCL),
 * and the servers' listening ports their clients connect to are published to
 * every engine.  Results equal shd_tcp_run's on the same model, host by host
 * (a client on another host than its server must start at least one window
 * after it, or the model is refused with -22, as on one engine).  Paths: with path_cache (every rank's own
 * cache of the same graph, built alike) each round's first-touch log of every
 * engine is gathered and replayed alike on every rank, so the ranks stay
 * equal and a contradicted choice stops every rank at the same round
 * (SHD_TCP_ERR_FIRST_TOUCH); with tables the queries every engine logged come
 * back in each rank's result, for the caller's ranking as on one engine.
 * Returns as shd_tcp_run, -5 also when the group's communication fails.
 * Failure is collective only where every rank sees it: an error bit of the
 * run, a halted engine (every engine ends at that round) and a first-touch
 * log too long for the device end every rank at the same round; a HIP error
 * local to one rank ends that rank's call, and the others stay in their next
 * collective until the transport gives up (the host transport after its
 * 300-s barrier timeout; RCCL does not time out). */
struct shd_comm;
int shd_tcp_run_group(const shd_tcp_model* m, struct shd_comm* comm, int32_t trace, shd_tcp_result** out);

/* keep != 0: shd_tcp_run keeps its device buffers (the per-host event queues,
 * packet pools, sockets and mailboxes: tens of GB at 64 k hosts) for the next
 * call on the same device instead of allocating and freeing them each call;
 * 0 (the default): release them now and after every call.  A caller that runs
 * many models in one process (a parameter sweep, the bench) sets 1. */
void shd_tcp_keep_workspace(int32_t keep);

/* The pcap files of captured hosts (utility/pcap_writer.c:19-137 restated
 * byte for byte; plain C, no device).  A file is the 24-byte global header
 * (0xA1B2C3D4, 2, 4, 0, 0, 65535, 1 in host byte order) and per record:
 * ts_sec = t / 10^9, ts_usec = (t % 10^9) / 1000, incl_len = orig_len = 66 +
 * payload; 14 Ethernet bytes (the two fixed MACs, 08 00); 20 IP bytes (45 00,
 * htons(orig_len - 14), 00 00, 40 00, 64, 6, 00 00, the addresses in network
 * order); 32 TCP bytes (the ports in network order, htonl(seq), htonl(ack)
 * when ACK is set and 0 otherwise, 80, the flag byte, htons((uint16_t)win),
 * 00 00, 14 zero bytes); the payload.  win is cut to 16 bits as the
 * reference's cast cuts it (network_interface.c:360-361).  The engine
 * simulates lengths, not content: payload bytes are zeros.
 * SHD_PCAP_HEADERS_ONLY: incl_len = 66, orig_len unchanged, no payload bytes.
 *
 * shd_pcap_format: the header (when with_header != 0) and the n records into
 * buf; returns the bytes needed, and writes only when cap holds them all
 * (buf NULL / cap 0: the size alone).
 * shd_pcap_write_host: writes <dir>/<hostname>-<a.b.c.d>.pcap
 * (network_interface.c:641-647; ip in host byte order) with the records, and
 * the host's loopback interface file <dir>/<hostname>-127.0.0.1.pcap with the
 * global header only (no model binds 127.0.0.1).  dir NULL: "data/pcapdata/"
 * (pcap_writer.c:150-153); the directory must exist.  Returns 0, -22 for
 * missing arguments, -2 when a file cannot be opened (the reference only
 * warns), -5 when a write fails. */
enum { SHD_PCAP_HEADERS_ONLY = 1 };
size_t shd_pcap_format(const shd_pcap_rec* recs, uint64_t n, uint32_t flags, int32_t with_header, uint8_t* buf,
                       size_t cap);
int shd_pcap_write_host(const char* dir, const char* hostname, uint32_t ip, const shd_pcap_rec* recs, uint64_t n,
                        uint32_t flags);

#ifdef __cplusplus
}
#endif
#endif
