// xyws_outbox.h — internal: rules 1 and 2 of xyws_outbox_streams (include/xyws.h),
// stated once for its plan pass (xyws_outbox.hip) and for the view that
// xyws_unsent_view_streams lays over a table (xyws_unsent.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "xyws.h"
#include "xyws_device.h"
#include "xyws_rows.h"

namespace xyws_internal {

// What a connection's row and the result rows it names say: full_len,
// len = min(full_len, out_cap) and the entry's flags (each thread's own loads).
struct outbox_lengths { uint64_t full, len; uint32_t flags; };
XYWS_DEV outbox_lengths outbox_rules(const xyws_rows::outbox_conn_row& c) {
  namespace rows = xyws_rows;
  uint32_t rst = 0, ast = 0, resp_len = 0, flags = 0;
  uint64_t reply_len = 0, full = 0;
  if (c.reply) {
    const rows::reply_result_row r = rows::load_reply_result<false>((const xyws_reply_result*)c.reply);
    reply_len = r.reply_len;
    rst = r.status;
  }
  if (c.accept) {
    const rows::accept_brief a = rows::load_accept_brief<false>((const xyws_accept_result*)c.accept);
    ast = a.status;
    resp_len = a.resp_len;
  }
  // rule 1: the last call of the sweep that wrote a row for it says what there is to send
  if (c.backlog) full = rows::load_backlog_send_len((const xyws_backlog_result*)c.backlog);
  else if (c.bcast) full = rows::load_bcast_result_own((const xyws_bcast_result*)c.bcast).send_len;
  else if (c.reply) full = reply_len;
  else if (ast & (XYWS_ACC_ACCEPTED | XYWS_ACC_REJECTED)) full = resp_len;
  // rule 2
  if ((rst & XYWS_RPL_CLOSED) || (ast & XYWS_ACC_REJECTED)) flags |= XYWS_OB_CLOSE;
  if (rst & XYWS_RPL_OVERFLOW) flags |= XYWS_OB_OVERFLOW;
  if (full > c.out_cap) flags |= XYWS_OB_TRUNCATED;
  return {full, full < c.out_cap ? full : c.out_cap, flags};
}

}  // namespace xyws_internal
