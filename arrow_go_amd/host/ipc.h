// Arrow IPC *stream* → record batches resident in HBM.
//
// What ipc.NewReader / Reader.Next do on the host (arrow/ipc/reader.go:97-120,202-300;
// message framing message.go:207-287; batch assembly file_reader.go:523-575, buffers :583-616,
// type decoding metadata.go) with one difference in where the bytes land: the body of a RecordBatch
// message is sent to the device with ONE copy and every column buffer becomes a slice of that one
// allocation — the IPC body is already laid out as Arrow buffers (8-byte aligned, validity / offsets /
// data in field order), so nothing is unpacked on the host.
//
// Both the stream format and the file format ("ARROW1" magic … footer) are read; the footer's block index is not
// needed for a sequential pass.
// Scope: flat columns of the types the kernels take — Int8..Uint64, Float32/64, Bool, Date32/64, Time32/64, Timestamp,
// Duration, Utf8 / Binary and their Large variants, plain or dictionary-encoded (DictionaryBatch messages, replacement and delta);
// little-endian; bodies uncompressed or compressed per buffer with LZ4_FRAME / ZSTD (ipc/compression.go: inflated on the host
// by the system's liblz4 / libzstd into the layout of an uncompressed body, then the same single transfer; an LZ4_FRAME body whose
// frames are made of independent 64 KiB blocks without checksums — lz4_frame.h decides frame by frame — is uploaded compressed and
// inflated in HBM into that same layout by ah_lz4_decompress_blocks, with the host path as the fall-back of every frame that does
// not qualify or that the device decoder reports a status for).  Anything else is
// ErrNotImplemented with the field named.  The metadata is a FlatBuffer (format/Message.fbs,
// Schema.fbs); it is read with the small bounds-checked accessor in ipc.cc — the bytes come from a
// file or a socket and are not trusted.
#pragma once
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "arrowhip_compute.h"
#include "lz4_frame.h"

namespace arrowhip {
namespace ipc {

struct FieldInfo {
  std::string name;
  const DataType* type = nullptr;        // the column's type; for a dictionary-encoded field the VALUE type
  std::string logical;                   // temporal columns: C Data format of the type, `type` is then the storage integer
  bool nullable = true;
  int64_t dict_id = -1;                  // ≥ 0: dictionary-encoded (Schema.fbs DictionaryEncoding.id)
  const DataType* index_type = nullptr;  // … with these indices on the wire
};

class StreamReader {
 public:
  // Parses the Schema message.  `bytes` must stay alive and unchanged while the reader is used.
  static Status Open(Session* s, const uint8_t* bytes, int64_t len, std::unique_ptr<StreamReader>* out);
  const std::vector<FieldInfo>& fields() const { return fields_; }
  // Next record batch: *have = false at the end of the stream (EOS marker or end of bytes).
  // columns == nullptr: only check the batch's metadata against its body (no session needed).
  Status Next(bool* have, std::vector<ArrayDataPtr>* columns, int64_t* rows);
  int64_t body_bytes_uploaded() const { return uploaded_; }
  // LZ4_FRAME bodies of at least min_bytes compressed bytes are inflated in HBM where their frames allow it (session options
  // ipc_device_lz4 / ipc_device_lz4_min_bytes); off: every compressed buffer is inflated on the host
  void set_device_lz4(bool on, int64_t min_bytes) { device_lz4_ = on; device_lz4_min_bytes_ = min_bytes; }
  // {bytes uploaded, buffers inflated on the device, buffers inflated on the host, buffers inflated on the host after a device status}
  void stats(int64_t out[4]) const { out[0] = uploaded_; out[1] = device_inflated_; out[2] = host_inflated_; out[3] = device_fallbacks_; }

 private:
  Status NextMessage(bool* have, const uint8_t** meta, int64_t* meta_len, const uint8_t** body, int64_t* body_len);
  // one RecordBatch table (a record batch message, or the `data` of a dictionary batch) against its body
  Status LoadColumns(const uint8_t* meta, int64_t meta_len, int64_t rb, const uint8_t* body, int64_t body_len,
                     const std::vector<FieldInfo>& fields, bool as_values, std::vector<ArrayDataPtr>* columns, int64_t* rows);
  // one buffer of a compressed body: [src, +srclen) of the body → [dst, +dstlen) of the plain layout; `blocks` if its frame was planned
  struct DevicePiece { int64_t src, srclen, dst, dstlen; bool stored, planned; std::vector<lz4::Block> blocks; };
  Status InflateOnDevice(const uint8_t* body, int64_t body_len, const std::vector<DevicePiece>& pieces, int64_t total, BufferPtr* dev);
  Status EnqueueInflate(const uint8_t* body, int64_t body_len, const std::vector<DevicePiece>& pieces, int64_t total, BufferPtr* dev,
                        BufferPtr* comp, std::vector<std::vector<uint8_t>>* host_bytes);
  bool device_lz4_ = true;
  int64_t device_lz4_min_bytes_ = 0, device_inflated_ = 0, host_inflated_ = 0, device_fallbacks_ = 0;
  std::map<int64_t, ArrayDataPtr> dicts_;   // dictionary id → values (dictutils.Memo)
  std::map<int64_t, bool> seen_dict_;
  Session* s_ = nullptr;
  const uint8_t* p_ = nullptr;
  int64_t n_ = 0, pos_ = 0, uploaded_ = 0;
  std::vector<FieldInfo> fields_;
};

// Record batches resident in HBM → an Arrow IPC stream (ipc.NewWriter / Writer.Write / Close, arrow/ipc/writer.go:85-260); the
// definition is in ipc_writer.cc and DESIGN.md §3.8.  The Schema message is written with the first batch, whose columns fix the
// fields: the types the reader above takes, plain or dictionary-encoded; anything else is ErrNotImplemented with the column named.
// A dictionary-encoded column gets a DictionaryBatch (isDelta = false) before the first record batch that uses it, and a
// replacement before any batch whose dictionary is not the identical device buffers of the one written last for that id.
// A column may be a slice: the bytes written are those of an offset-0 array of its rows.  Every byte of the stream is defined.
// With lz4 every buffer is an LZ4 frame of independent 64 KiB blocks without checksums — what the reader's device path accepts —
// compressed in HBM, or its raw bytes behind a −1 prefix where the frame would not be smaller; a buffer of no bytes has length 0.
// A Write that fails appends nothing (the first one may leave the Schema message) and the writer stays usable.
class StreamWriter {
 public:
  StreamWriter(Session* s, bool lz4);
  Status Write(const std::vector<std::string>& names, const std::vector<ArrayDataPtr>& columns);
  Status Close();   // the end-of-stream marker; Write is refused afterwards
  const std::vector<uint8_t>& bytes() const { return out_; }
  // {plain bytes of all buffers, body bytes written, buffers written as frames, buffers written raw behind −1} so far
  void stats(int64_t out[4]) const { for (int i = 0; i < 4; i++) out[i] = stats_[i]; }

 private:
  struct Piece;
  struct Column;
  struct Message;
  Status Describe(const std::string& name, const ArrayData& a, int64_t next_dict_id, FieldInfo* out) const;
  Status WriteSchema();
  Session* s_;
  bool lz4_, have_schema_ = false, closed_ = false;
  std::vector<FieldInfo> fields_;
  std::map<int64_t, ArrayDataPtr> written_dicts_;   // dictionary id → the dictionary written last (kept alive: see SameBuffers)
  std::vector<uint8_t> out_;
  int64_t stats_[4] = {0, 0, 0, 0};
};

}  // namespace ipc
}  // namespace arrowhip
