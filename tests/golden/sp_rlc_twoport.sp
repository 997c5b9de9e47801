* lossy low-pass section: series R + L from port 1, shunt C with a loss resistor at port 2
V1 p1 0 DC 0 PORTNUM 1 Z0 50
V2 p2 0 DC 0 PORTNUM 2 Z0 50
RS p1 m 2
L1 m p2 100n
C1 p2 0 20p
RP p2 0 2k
.SP DEC 4 10meg 1g
