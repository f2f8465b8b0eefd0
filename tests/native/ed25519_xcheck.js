// Node cross-check of Ed25519 verdicts (tests/test_ed25519_cpu.py): the same record stream as
// ed25519_xcheck.c on stdin, one character '0' / '1' per record on stdout.
const crypto = require("crypto");
const chunks = [];
process.stdin.on("data", (c) => chunks.push(c));
process.stdin.on("end", () => {
  const buf = Buffer.concat(chunks);
  // SubjectPublicKeyInfo prefix of an Ed25519 key (RFC 8410): the raw 32 bytes follow
  const spki = Buffer.from("302a300506032b6570032100", "hex");
  let out = "";
  for (let p = 0; p + 98 <= buf.length; ) {
    const len = buf.readUInt16LE(p + 96);
    const pub = buf.slice(p, p + 32), sig = buf.slice(p + 32, p + 96), msg = buf.slice(p + 98, p + 98 + len);
    p += 100 + len;
    let ok = false;
    try {
      const key = crypto.createPublicKey({ key: Buffer.concat([spki, pub]), format: "der", type: "spki" });
      ok = crypto.verify(null, msg, key, sig);
    } catch (e) {
      ok = false;
    }
    out += ok ? "1" : "0";
  }
  console.log(out);
});
